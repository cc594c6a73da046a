"""Mirror of jepsen.checker/perf's analysis (etcdemo.clj:165-167).

    checker.perf()   (checker/perf): always {"valid?": True}.  What Jepsen
                     computes before it calls gnuplot is computed on the device:
                     the latency of every completed client op, latency quantiles
                     per (:f, 30 s window) and completion rates per (:f, :type,
                     10 s window).  With test["store-path"] set, the series are
                     written there as latency-quantiles.tsv and rate.tsv.  No
                     image is drawn.

The path is its own: PerfHistory (lc_perf_history) -> PackedPerf (lc_perf_pack:
pairing, orphans, nemesis intervals on the host) -> lc_perf_check -> series.
The rules are stated in DESIGN.md section 3.10.  With {"pack": "device"} the
rows are paired and packed on the device as well (CheckedPerf:
lc_perf_check_history); the series are the same.
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

TYPES = {"invoke": N.LC_INVOKE, "ok": N.LC_OK_T, "fail": N.LC_FAIL, "info": N.LC_INFO}
TYPE_NAMES = {v: k for k, v in TYPES.items()}
COMPLETIONS = ("ok", "fail", "info")  # the rate table's type order


def _name(x) -> str:
    return "nil" if x is None else str(x).lstrip(":")


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


class PerfHistory:
    """A whole history as the four columns perf reads (lc_perf_history) and the
    table of :f names the f column indexes."""

    def __init__(self, type_, f, process, time, names: Sequence[str]):
        self.type = np.ascontiguousarray(type_, np.uint8)
        self.f = np.ascontiguousarray(f, np.uint8)
        self.process = np.ascontiguousarray(process, np.int64)
        self.time = np.ascontiguousarray(time, np.int64)
        self.names = [str(x) for x in names]
        self.n = len(self.type)
        if not (len(self.f) == len(self.process) == len(self.time) == self.n):
            raise ValueError("PerfHistory: columns of different lengths")

    @classmethod
    def from_ops(cls, ops: Sequence[dict]) -> "PerfHistory":
        """Op maps ({"type", "f", "process", "time"}; :value is not read) to
        columns, by the rules of lc_edn_read_perf: names interned in order of
        first appearance, a :process that is no integer is LC_NO_PROCESS."""
        n = len(ops)
        type_, f = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        process, time = np.full(n, N.LC_NO_PROCESS, np.int64), np.zeros(n, np.int64)
        ids: Dict[str, int] = {}
        for r, op in enumerate(ops):
            type_[r] = TYPES[_name(op["type"])]
            name = _name(op.get("f"))
            if name not in ids:
                if len(ids) >= 256:
                    raise ValueError("more than 256 distinct :f")
                ids[name] = len(ids)
            f[r] = ids[name]
            if _is_int(op.get("process")):
                process[r] = int(op["process"])
            t = op.get("time")
            if not _is_int(t):
                raise ValueError(f"op {r}: no integer :time")
            time[r] = int(t)
        return cls(type_, f, process, time, list(ids))

    @classmethod
    def read_edn(cls, path: str) -> "PerfHistory":
        """lc_edn_read_perf: any Jepsen history.edn."""
        h = C.c_void_p()
        N.check(N.lib().lc_edn_read_perf(str(path).encode(), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_perf_hist_free(h)

    @classmethod
    def parse_edn(cls, text: str) -> "PerfHistory":
        data = text.encode()
        h = C.c_void_p()
        N.check(N.lib().lc_edn_parse_perf(data, len(data), C.byref(h)))
        try:
            return cls._from_handle(h)
        finally:
            N.lib().lc_perf_hist_free(h)

    @classmethod
    def _from_handle(cls, h) -> "PerfHistory":
        v = N.LcPerfHistory()
        N.check(N.lib().lc_perf_hist_view(h, C.byref(v)))
        n = int(v.n)
        names = [N.lib().lc_perf_hist_name(h, i).decode(errors="replace") for i in range(int(v.n_f))]
        return cls(N.carray(v.type, n, np.uint8), N.carray(v.f, n, np.uint8), N.carray(v.process, n, np.int64),
                   N.carray(v.time, n, np.int64), names)

    def f_id(self, name: str) -> int:
        return self.names.index(name) if name in self.names else -1

    def as_c(self) -> N.LcPerfHistory:
        return N.LcPerfHistory(self.n, N.ptr(self.type, C.c_uint8), N.ptr(self.f, C.c_uint8),
                               N.ptr(self.process, C.c_int64), N.ptr(self.time, C.c_int64), len(self.names),
                               self.f_id("start"), self.f_id("stop"))

    def to_ops(self) -> List[dict]:
        """The rows as op maps again (tests; small histories)."""
        return [{"type": TYPE_NAMES[int(self.type[r])], "f": self.names[int(self.f[r])],
                 "process": "nemesis" if self.process[r] == N.LC_NO_PROCESS else int(self.process[r]),
                 "time": int(self.time[r])} for r in range(self.n)]


class PackedPerf:
    """lc_perf_pack output: one record per client completion, the nemesis
    intervals and the pairing counts."""

    def __init__(self, hist: PerfHistory):
        self.hist = hist
        self.names = list(hist.names)
        self._c = hist.as_c()
        h = C.c_void_p()
        N.check(N.lib().lc_perf_pack(C.byref(self._c), C.byref(h)))
        self.handle = h
        v = N.LcPerfBatch()
        N.check(N.lib().lc_perf_packed_view(h, C.byref(v)))
        self.view = v
        self.n = int(v.n)
        info = np.zeros(4, np.int64)
        N.check(N.lib().lc_perf_packed_info(h, N.ptr(info, C.c_int64)))
        self.matched, self.unmatched, self.orphans, n_iv = (int(x) for x in info)
        iv = np.zeros(max(2 * n_iv, 2), np.int64)
        N.check(N.lib().lc_perf_packed_intervals(h, N.ptr(iv, C.c_int64)))
        self.intervals = iv[:2 * n_iv].reshape(n_iv, 2)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_perf_packed_free(h)
            self.handle = None

    def arrays(self) -> Dict[str, np.ndarray]:
        """Copies of the record columns: t_comp, t_inv, f_inv, f_comp, type."""
        v = self.view
        meta = N.carray(v.meta, self.n, np.uint32)
        return dict(t_comp=N.carray(v.t_comp, self.n, np.int64), t_inv=N.carray(v.t_inv, self.n, np.int64), meta=meta,
                    f_inv=(meta & 0xFF).astype(np.uint8), f_comp=((meta >> 8) & 0xFF).astype(np.uint8),
                    type=((meta >> 16) & 0xFF).astype(np.uint8))


PACKS = ("host", "device")


def pack_of(opts: Optional[Dict]) -> str:
    """The {"pack": ...} option: "host" (the default) or "device"."""
    pack = (opts or {}).get("pack", "host")
    if pack not in PACKS:
        raise ValueError(f'"pack" is "host" or "device", not {pack!r}')
    return pack


class CheckedPerf:
    """lc_perf_check_history output: what PerfSeries reads from a PackedPerf
    (names, intervals, the pairing counts, arrays()) and lc_perf_check's tables,
    from one call that pairs and packs the rows on the device.  arrays()
    downloads the record columns on first use; the device keeps them only until
    the context's next perf call."""

    def __init__(self, dev, hist: PerfHistory, opts: Optional[N.LcPerfOpts] = None):
        self.dev, self.hist = dev, hist
        self.names = list(hist.names)
        self._c = hist.as_c()
        o = opts if opts is not None else make_opts()
        h = C.c_void_p()
        N.check(N.lib().lc_perf_check_history(dev.handle, C.byref(self._c), C.byref(o), C.byref(h)))
        self.handle = h
        v, r = N.LcPerfBatch(), N.LcPerfResult()
        N.check(N.lib().lc_perf_checked_view(h, C.byref(v), C.byref(r)))
        self.view = v
        self.n = int(v.n)
        info = np.zeros(4, np.int64)
        N.check(N.lib().lc_perf_checked_info(h, N.ptr(info, C.c_int64)))
        self.matched, self.unmatched, self.orphans, n_iv = (int(x) for x in info)
        iv = np.zeros(max(2 * n_iv, 2), np.int64)
        N.check(N.lib().lc_perf_checked_intervals(h, N.ptr(iv, C.c_int64)))
        self.intervals = iv[:2 * n_iv].reshape(n_iv, 2)
        ms = (C.c_double * 6)()
        N.check(N.lib().lc_perf_history_timing(dev.handle, ms))
        F, nr, nq, n_q = int(v.n_f), int(r.rate_n), int(r.q_n), int(o.n_q)
        self.results = PerfResults(
            F, tuple(o.q[j] for j in range(n_q)), int(o.rate_dt_ns), int(o.quantile_dt_ns), int(r.rate_first), int(r.q_first),
            N.carray(r.rate, F * 3 * nr, np.uint64).reshape(F, 3, nr), N.carray(r.group, F * nq, np.uint64).reshape(F, nq),
            N.carray(r.quant, F * nq * n_q, np.int64).reshape(F, nq, n_q),
            dict(upload_ms=ms[0], pair_ms=ms[1], build_ms=ms[2], kernel_ms=ms[3], download_ms=ms[4], total_ms=ms[5]))
        self._arrays = None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            N.lib().lc_perf_checked_free(h)
            self.handle = None

    def arrays(self) -> Dict[str, np.ndarray]:
        """Copies of the record columns, as PackedPerf.arrays()."""
        if self._arrays is None:
            b = N.LcPerfBatch()
            N.check(N.lib().lc_perf_checked_records(self.dev.handle, self.handle, C.byref(b)))
            meta = N.carray(b.meta, self.n, np.uint32)
            self._arrays = dict(t_comp=N.carray(b.t_comp, self.n, np.int64), t_inv=N.carray(b.t_inv, self.n, np.int64), meta=meta,
                                f_inv=(meta & 0xFF).astype(np.uint8), f_comp=((meta >> 8) & 0xFF).astype(np.uint8),
                                type=((meta >> 16) & 0xFF).astype(np.uint8))
        return self._arrays


def batch_of(arrs: Dict[str, Any], n_f: int) -> N.LcPerfBatch:
    """An lc_perf_batch over numpy columns t_comp, t_inv, meta (a caller's own;
    the bounds and the matched count are computed here).  The arrays must
    outlive the call that reads the batch."""
    tc = np.ascontiguousarray(arrs["t_comp"], np.int64)
    ti = np.ascontiguousarray(arrs["t_inv"], np.int64)
    meta = np.ascontiguousarray(arrs["meta"], np.uint32)
    n = len(tc)
    m = ti != N.LC_PERF_NO_INVOKE
    nm = int(m.sum())
    pad = [a if len(a) else np.zeros(1, a.dtype) for a in (tc, ti, meta)]
    arrs["_keep"] = pad
    return N.LcPerfBatch(n, N.ptr(pad[0], C.c_int64), N.ptr(pad[1], C.c_int64), N.ptr(pad[2], C.c_uint32), nm,
                         int(tc.min()) if n else 0, int(tc.max()) if n else 0, int(ti[m].min()) if nm else 0,
                         int(ti[m].max()) if nm else 0, int(n_f), 0)


def make_opts(opts: Optional[Dict] = None) -> N.LcPerfOpts:
    """lc_perf_opts from {"quantile-dt-ns", "rate-dt-ns", "quantiles", "flags"};
    whatever is missing keeps Jepsen's default."""
    opts = opts or {}
    o = N.LcPerfOpts()
    N.lib().lc_perf_opts_default(C.byref(o))
    if opts.get("quantile-dt-ns") is not None:
        o.quantile_dt_ns = int(opts["quantile-dt-ns"])
    if opts.get("rate-dt-ns") is not None:
        o.rate_dt_ns = int(opts["rate-dt-ns"])
    if opts.get("quantiles") is not None:
        qs = [float(q) for q in opts["quantiles"]]
        if not 1 <= len(qs) <= N.LC_PERF_MAX_Q:
            raise ValueError(f"1 to {N.LC_PERF_MAX_Q} quantiles")
        o.n_q = len(qs)
        for j, q in enumerate(qs):
            o.q[j] = q
    o.flags = int(opts.get("flags", 0))
    return o


@dataclass
class PerfResults:
    """lc_perf_check's tables."""
    n_f: int
    qs: Tuple[float, ...]
    rate_dt_ns: int
    quantile_dt_ns: int
    rate_first: int
    q_first: int
    rate: np.ndarray   # uint64 [n_f, 3, rate_n]: ok, fail, info
    group: np.ndarray  # uint64 [n_f, q_n]
    quant: np.ndarray  # int64 [n_f, q_n, n_q] latencies, ns
    timing: Dict[str, float] = field(default_factory=dict)


def check_batch(dev, batch: N.LcPerfBatch, opts: Optional[N.LcPerfOpts] = None) -> PerfResults:
    """lc_perf_check on a checker.Device."""
    o = opts if opts is not None else make_opts()
    shape = np.zeros(4, np.int64)
    N.check(N.lib().lc_perf_shape(C.byref(batch), C.byref(o), N.ptr(shape, C.c_int64)))
    F, nr, nq, n_q = int(batch.n_f), int(shape[1]), int(shape[3]), int(o.n_q)
    rate, group = np.zeros(max(F * 3 * nr, 1), np.uint64), np.zeros(max(F * nq, 1), np.uint64)
    quant = np.zeros(max(F * nq * n_q, 1), np.int64)
    r = N.LcPerfResult(N.ptr(rate, C.c_uint64), N.ptr(group, C.c_uint64), N.ptr(quant, C.c_int64), len(rate), len(group),
                       len(quant), 0, 0, 0, 0)
    N.check(N.lib().lc_perf_check(dev.handle, C.byref(batch), C.byref(o), C.byref(r)))
    ms = (C.c_double * 4)()
    N.check(N.lib().lc_perf_last_timing(dev.handle, ms))
    return PerfResults(F, tuple(o.q[j] for j in range(n_q)), int(o.rate_dt_ns), int(o.quantile_dt_ns), int(r.rate_first),
                       int(r.q_first), rate[:F * 3 * nr].reshape(F, 3, nr), group[:F * nq].reshape(F, nq),
                       quant[:F * nq * n_q].reshape(F, nq, n_q),
                       dict(upload_ms=ms[0], kernel_ms=ms[1], download_ms=ms[2], total_ms=ms[3]))


class PerfSeries:
    """The series jepsen.checker.perf hands to gnuplot.

        quantiles[f][q]  [(t_mid_s, latency_ms)]  one point per non-empty window
        rate[f][type]    [(t_mid_s, per_s)]       one point per non-empty window
        nemesis          [(t0_s, t1_s)]
        points(f, type)  [(t_s, latency_ms)] of every completed op, from the pack
    """

    def __init__(self, packed, res: PerfResults):
        self.packed, self.res = packed, res
        self.names = packed.names
        self.quantiles: Dict[str, Dict[float, List[Tuple[float, float]]]] = {}
        self.rate: Dict[str, Dict[str, List[Tuple[float, float]]]] = {}
        qdt, rdt = res.quantile_dt_ns, res.rate_dt_ns
        for fi, name in enumerate(self.names):
            live = np.nonzero(res.group[fi])[0] if res.group.size else []
            if len(live):
                mids = ((res.q_first + live) * qdt + qdt // 2) / 1e9
                self.quantiles[name] = {q: list(zip(mids.tolist(), (res.quant[fi, live, j] / 1e6).tolist()))
                                        for j, q in enumerate(res.qs)}
            by_type = {}
            for ti, tname in enumerate(COMPLETIONS):
                row = res.rate[fi, ti] if res.rate.size else np.zeros(0, np.uint64)
                nz = np.nonzero(row)[0]
                if len(nz):
                    mids = ((res.rate_first + nz) * rdt + rdt // 2) / 1e9
                    by_type[tname] = list(zip(mids.tolist(), (row[nz] / (rdt / 1e9)).tolist()))
            if by_type:
                self.rate[name] = by_type
        self.nemesis = [(a / 1e9, b / 1e9) for a, b in packed.intervals.tolist()]
        self._arrays = None

    def points(self, f: str, type_: str) -> List[Tuple[float, float]]:
        """Jepsen's latency points of (:f, completion :type), in history order."""
        if self._arrays is None:
            self._arrays = self.packed.arrays()
        a = self._arrays
        if f not in self.names:
            return []
        m = (a["t_inv"] != N.LC_PERF_NO_INVOKE) & (a["f_inv"] == self.names.index(f)) & (a["type"] == TYPES[type_])
        x, lat = a["t_inv"][m], a["t_comp"][m] - a["t_inv"][m]
        return list(zip((x / 1e9).tolist(), (lat / 1e6).tolist()))

    def quantile_rows(self):
        """(series name, x, y) rows of latency-quantiles.tsv."""
        for name, by_q in self.quantiles.items():
            for q, pts in by_q.items():
                for x, y in pts:
                    yield f"{name} {q:g}", x, y

    def rate_rows(self):
        for name, by_t in self.rate.items():
            for t, pts in by_t.items():
                for x, y in pts:
                    yield f"{name} {t}", x, y


def analyze(dev, history, opts: Optional[Dict] = None) -> PerfSeries:
    """The perf series of a whole history (a PerfHistory or op maps) on a
    checker.Device.  opts["pack"]: "host" (lc_perf_pack, then lc_perf_check) or
    "device" (lc_perf_check_history)."""
    pack = pack_of(opts)
    hist = history if isinstance(history, PerfHistory) else PerfHistory.from_ops(history)
    if pack == "device":
        checked = CheckedPerf(dev, hist, make_opts(opts))
        return PerfSeries(checked, checked.results)
    packed = PackedPerf(hist)
    return PerfSeries(packed, check_batch(dev, packed.view, make_opts(opts)))


def write_tsv(path: str, rows) -> None:
    with open(path, "w") as f:
        for name, x, y in rows:
            f.write(f"{name}\t{x!r}\t{y!r}\n")


class PerfChecker:
    """jepsen.checker/perf: {"valid?": True}, the series written as a side
    effect when the test has a store."""

    def __init__(self, opts: Optional[Dict] = None):
        self.opts = dict(opts or {})
        self.pack = pack_of(self.opts)
        self.device = int(self.opts.get("device", 0))
        self.last: Optional[PerfSeries] = None

    def _dev(self):
        from . import checker as ck
        return ck.device_for(self.device)

    def check(self, test: Optional[Dict], history, opts: Optional[Dict] = None) -> Dict:
        hist = history if isinstance(history, PerfHistory) else PerfHistory.from_ops(history)
        series = analyze(self._dev(), hist, self.opts)
        self.last = series
        store = (test or {}).get("store-path")
        if store:
            sub = [str(d) for d in (opts or {}).get("subdirectory", [])]
            out = os.path.join(store, *sub)
            os.makedirs(out, exist_ok=True)
            write_tsv(os.path.join(out, "latency-quantiles.tsv"), series.quantile_rows())
            write_tsv(os.path.join(out, "rate.tsv"), series.rate_rows())
        return {"valid?": True}


def perf(opts: Optional[Dict] = None) -> PerfChecker:
    return PerfChecker(opts)
