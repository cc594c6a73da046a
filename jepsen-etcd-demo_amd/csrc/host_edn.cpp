// history.edn reader / writer (native Jepsen history
// ingestion; the store/ layout the demo writes, .gitignore:13, and that
// `lein run analyze` re-checks).
//
// Input: the op maps Jepsen writes, one per line or inside one vector, e.g.
//   {:type :invoke, :f :cas, :value [3 [1 4]], :process 7, :time 1234, :index 12}
//   {:type :info, :f :start, :value nil, :process :nemesis, :time 99, :index 13}
// Fields read: :type :f :process :value :index.  Every other field (and any
// EDN value: maps, sets, lists, strings, chars, tagged literals, metadata) is
// skipped by a generic reader.
//
// Independent tuples: EDN prints a jepsen.independent tuple (a MapEntry) as a
// plain [k v] vector, so the reader decides per history: if every client op
// (:f :read/:write/:cas) has a 2-element vector value, values are [k v]
// tuples (the register workload, etcdemo.clj:90, :120); otherwise values are
// used as they are.

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <string>
#include <string_view>
#include <system_error>
#include <thread>
#include <unordered_map>

#include "common.hpp"

// Parsing is allocation-free per op (string_view tokens, fixed-depth value
// records) and, for the one-op-per-line form, split at line starts over up to
// 16 threads whose row blocks are concatenated in order.  Anything the split
// could misread (an op map spanning a line break inside a string) fails its
// chunk, and the whole text is then re-read serially, which gives the exact
// result or error.  LC_EDN_THREADS caps the thread count (1 = serial).

namespace {

enum : uint8_t { K_NIL, K_INT, K_VEC, K_OTHER };

// A :value, only as deep as the register workloads need: [k [a b]].
struct Leaf { uint8_t kind = K_OTHER; int64_t i = 0; };
struct Node { uint8_t kind = K_OTHER; int64_t i = 0; uint32_t n = 0; Leaf e[2]; };
struct Top { uint8_t kind = K_OTHER; int64_t i = 0; uint32_t n = 0; Node e[2]; };

struct Delims {
    bool d[256] = {};
    Delims() {
        for (unsigned char c : std::string_view(" \t\n\r,)]}([{\";")) d[c] = true;
    }
};
const Delims DELIM;

// A token of up to 8 bytes as one little-endian word (longer: ~0), so that
// keyword and symbol comparisons are integer compares, not library calls.
inline uint64_t pack8(std::string_view t) {
    if (t.size() > 8) return ~0ull;
    uint64_t x = 0;
    for (size_t i = 0; i < t.size(); ++i) x |= (uint64_t)(unsigned char)t[i] << (8 * i);
    return x;
}
template <size_t N>
constexpr uint64_t P8(const char (&s)[N]) {
    static_assert(N - 1 <= 8, "P8: at most 8 bytes");
    uint64_t x = 0;
    for (size_t i = 0; i + 1 < N; ++i) x |= (uint64_t)(unsigned char)s[i] << (8 * i);
    return x;
}

struct Parser {
    const char *p, *end, *base;
    std::string err;
    size_t err_off = 0;

    bool fail(const std::string &m) {
        if (err.empty()) { err = m; err_off = (size_t)(p - base); }
        return false;
    }
    void ws() {
        while (p < end) {
            const char c = *p;
            if (c == ' ' || c == ',' || c == '\n' || c == '\t' || c == '\r') ++p;
            else if (c == ';') { while (p < end && *p != '\n') ++p; }
            else break;
        }
    }
    std::string_view token() {
        const char *s = p;
        while (p < end && !DELIM.d[(unsigned char)*p]) ++p;
        return std::string_view(s, (size_t)(p - s));
    }
    bool string_lit() {
        ++p;
        while (p < end && *p != '"') p += (*p == '\\') ? 2 : 1;
        if (p >= end) return fail("unterminated string");
        ++p;
        return true;
    }
    // Metadata (^m) and discards (#_ x) in front of a value.
    bool prefixes() {
        ws();
        if (p < end && *p != '^' && *p != '#') return true;  // the common case
        for (;;) {
            ws();
            if (p >= end) return fail("unexpected end of input");
            if (*p == '^') { ++p; if (!skip()) return false; continue; }
            if (*p == '#' && p + 1 < end && p[1] == '_') { p += 2; if (!skip()) return false; continue; }
            return true;
        }
    }
    bool skip_seq(char close) {
        ++p;
        for (;;) {
            ws();
            if (p >= end) return fail("unterminated collection");
            if (*p == close) { ++p; return true; }
            if (!skip()) return false;
        }
    }
    // Read one scalar token (number / nil / true / false / symbol).
    bool scalar(uint8_t &kind, int64_t &v) {
        // the common case first: a decimal integer of at most 18 digits
        // followed by a delimiter (no overflow possible)
        {
            const char *q = p;
            const bool neg = q < end && *q == '-';
            if (q < end && (*q == '-' || *q == '+')) ++q;
            const char *d0 = q;
            uint64_t acc = 0;
            while (q < end && q - d0 < 18 && (unsigned)(*q - '0') < 10u) acc = acc * 10 + (uint64_t)(*q++ - '0');
            if (q > d0 && (q == end || DELIM.d[(unsigned char)*q])) {
                const int64_t val = neg ? -(int64_t)acc : (int64_t)acc;
                if (val != LC_NIL) {
                    p = q;
                    kind = K_INT;
                    v = val;
                    return true;
                }
            }
        }
        const char c = *p;
        std::string_view t = token();
        kind = K_OTHER;
        if (t.empty()) return fail(std::string("unexpected character '") + c + "'");
        if (pack8(t) == P8("nil")) { kind = K_NIL; return true; }
        const char f0 = t[0];
        const bool num = (f0 >= '0' && f0 <= '9') || ((f0 == '-' || f0 == '+') && t.size() > 1 && t[1] >= '0' && t[1] <= '9');
        if (!num) return true;  // true / false / symbol
        std::string_view d = t;
        if (d.back() == 'N' || d.back() == 'M') d.remove_suffix(1);
        if (d.find_first_of(".eE/") != std::string_view::npos) return true;  // not integral
        bool neg = false;
        size_t j = 0;
        if (d[0] == '-' || d[0] == '+') { neg = d[0] == '-'; j = 1; }
        unsigned __int128 acc = 0;
        for (; j < d.size(); ++j) {
            const char x = d[j];
            if (x < '0' || x > '9') return fail("integer out of range: " + std::string(t));
            acc = acc * 10 + (unsigned)(x - '0');
            if (acc > (unsigned __int128)INT64_MAX + 1) return fail("integer out of range: " + std::string(t));
        }
        if (!neg && acc > (unsigned __int128)INT64_MAX) return fail("integer out of range: " + std::string(t));
        const int64_t val = neg ? (int64_t)(0 - (uint64_t)acc) : (int64_t)acc;
        if (val == LC_NIL) return fail("integer reserved for nil: " + std::string(t));
        kind = K_INT;
        v = val;
        return true;
    }
    // Skip one value of any EDN kind.
    bool skip() {
        if (!prefixes()) return false;
        switch (*p) {
            case '[': return skip_seq(']');
            case '(': return skip_seq(')');
            case '{': return skip_seq('}');
            case '"': return string_lit();
            case '\\': ++p; if (p < end) ++p; token(); return true;  // char literal
            case ':': ++p; token(); return true;
            case '#': {
                ++p;
                if (p < end && *p == '{') return skip_seq('}');  // set
                if (p < end && *p == '"') return string_lit();   // regex
                token();                                         // tagged literal
                return skip();
            }
            default: {
                uint8_t k;
                int64_t v;
                return scalar(k, v);
            }
        }
    }
    // A value whose shape we keep: scalars, and vectors down to `depth`.
    template <class V>
    bool shaped(V &out);
    bool keyword(std::string_view &kw, bool &is_kw) {
        if (!prefixes()) return false;
        is_kw = *p == ':';
        if (!is_kw) return skip();
        ++p;
        kw = token();
        return true;
    }
};

template <class V>
bool Parser::shaped(V &out) {
    if (!prefixes()) return false;
    out.kind = K_OTHER;
    const char c = *p;
    if (c == '[') {
        out.kind = K_VEC;
        out.n = 0;
        ++p;
        for (;;) {
            ws();
            if (p >= end) return fail("unterminated collection");
            if (*p == ']') { ++p; return true; }
            bool ok;
            if constexpr (sizeof(V) == sizeof(Leaf)) {
                ok = skip();
            } else {
                if (out.n < 2) ok = shaped(out.e[out.n]);
                else ok = skip();
            }
            if (!ok) return false;
            ++out.n;
        }
    }
    if (c == '(' || c == '{' || c == '"' || c == '\\' || c == ':' || c == '#') return skip();
    return scalar(out.kind, out.i);
}
template <>
bool Parser::shaped<Leaf>(Leaf &out) {
    if (!prefixes()) return false;
    out.kind = K_OTHER;
    const char c = *p;
    if (c == '[' || c == '(' || c == '{' || c == '"' || c == '\\' || c == ':' || c == '#') return skip();
    return scalar(out.kind, out.i);
}

struct RawOp {
    uint8_t type = 255, f = LC_F_OTHER;
    int8_t nem = -1;  // nemesis :f :start (1) / :stop (0)
    int64_t process = LC_NO_PROCESS, index = -1;
    Top value;
    const char *vb = nullptr;  // where the :value's text starts (a :txn value is read again from there)
};

// Register names of :txn micro-ops, interned in order of first appearance.
struct Names {
    std::unordered_map<std::string, int64_t> id;
    std::vector<std::string> names;
    int64_t of(std::string_view t) {
        auto it = id.find(std::string(t));
        if (it != id.end()) return it->second;
        const int64_t v = LC_NAMED_REG_BASE + (int64_t)names.size();
        names.emplace_back(t);
        id.emplace(names.back(), v);
        return v;
    }
};

// A :txn op's value is [k txn] (an independent tuple) when its first element
// is an integer; a txn of two micro-ops starts with a vector instead.
bool txn_tuple(const Top &v) { return v.kind == K_VEC && v.n == 2 && v.e[0].kind == K_INT; }

// The op-map keys read, by length and spelling (one compare per key).
enum Field { FLD_OTHER, FLD_TYPE, FLD_F, FLD_PROCESS, FLD_INDEX, FLD_VALUE };
inline Field field_of(std::string_view k) {
    switch (pack8(k)) {
        case P8("f"): return FLD_F;
        case P8("type"): return FLD_TYPE;
        case P8("value"): return FLD_VALUE;
        case P8("index"): return FLD_INDEX;
        case P8("process"): return FLD_PROCESS;
        default: return FLD_OTHER;
    }
}

bool read_op(Parser &ps, RawOp &op) {
    ++ps.p;  // at '{'
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated op map");
        if (*ps.p == '}') { ++ps.p; break; }
        std::string_view k;
        bool is_kw = false;
        if (!ps.keyword(k, is_kw)) return false;
        if (!is_kw) {  // non-keyword key: skip its value
            if (!ps.skip()) return false;
            continue;
        }
        const Field fld = field_of(k);
        if (fld == FLD_TYPE || fld == FLD_F) {
            std::string_view v;
            bool vk = false;
            if (!ps.keyword(v, vk)) return false;
            if (fld == FLD_TYPE) {
                if (!vk) return ps.fail(":type is not a keyword");
                switch (pack8(v)) {
                    case P8("invoke"): op.type = LC_INVOKE; break;
                    case P8("ok"): op.type = LC_OK_T; break;
                    case P8("fail"): op.type = LC_FAIL; break;
                    case P8("info"): op.type = LC_INFO; break;
                    default: return ps.fail("unknown :type :" + std::string(v));
                }
            } else {
                op.f = LC_F_OTHER;
                op.nem = -1;
                if (vk) {
                    switch (pack8(v)) {
                        case P8("read"): op.f = LC_F_READ; break;
                        case P8("write"): op.f = LC_F_WRITE; break;
                        case P8("cas"): op.f = LC_F_CAS; break;
                        case P8("acquire"): op.f = LC_F_ACQUIRE; break;  // (model/mutex)
                        case P8("release"): op.f = LC_F_RELEASE; break;
                        case P8("txn"): op.f = LC_F_TXN; break;          // (model/multi-register)
                        case P8("start"): op.nem = 1; break;             // nemesis
                        case P8("stop"): op.nem = 0; break;
                        default: break;
                    }
                }
            }
        } else if (fld == FLD_PROCESS || fld == FLD_INDEX) {
            Leaf v;
            if (!ps.shaped(v)) return false;
            if (fld == FLD_PROCESS) op.process = v.kind == K_INT ? v.i : LC_NO_PROCESS;
            else op.index = v.kind == K_INT ? v.i : -1;
        } else if (fld == FLD_VALUE) {
            if (!ps.prefixes()) return false;
            op.vb = ps.p;
            if (!ps.shaped(op.value)) return false;
        } else {
            if (!ps.skip()) return false;
        }
    }
    if (op.type == 255) return ps.fail("op map without :type");
    return true;
}

enum { CONV_OK = 0, CONV_KEY = 1, CONV_VALUE = 2, CONV_TXN = 3 };

// One micro-op [f k v]: f :read/:write (or :r/:w), k an integer or a name,
// v an integer or nil.
bool micro_op(Parser &ps, Names &names, std::vector<int64_t> &out) {
    if (!ps.prefixes() || *ps.p != '[') return false;
    ++ps.p;
    std::string_view f;
    bool fk = false;
    if (!ps.keyword(f, fk) || !fk) return false;
    int64_t code;
    if (f == "read" || f == "r") code = LC_MOP_READ;
    else if (f == "write" || f == "w") code = LC_MOP_WRITE;
    else return false;
    if (!ps.prefixes()) return false;
    int64_t reg;
    const char c = *ps.p;
    if (c == ':' || c == '"' || (c != '-' && c != '+' && (c < '0' || c > '9'))) {
        const char *b = ps.p;
        if (!ps.skip()) return false;
        const std::string_view t(b, (size_t)(ps.p - b));
        if (t == "nil" || t.empty()) return false;
        reg = names.of(t);
    } else {
        uint8_t kind;
        if (!ps.scalar(kind, reg) || kind != K_INT || reg >= LC_NAMED_REG_BASE) return false;
    }
    Leaf v;
    if (!ps.shaped(v) || (v.kind != K_INT && v.kind != K_NIL)) return false;
    const int64_t val = v.kind == K_NIL ? LC_NIL : v.i;
    if (val == LC_NIL + 1) return false;  // the multi-register model's "absent"
    ps.ws();
    if (ps.p >= ps.end || *ps.p != ']') return false;
    ++ps.p;
    out.push_back(code);
    out.push_back(reg);
    out.push_back(val);
    return true;
}

// A :txn value (nil, or a vector of micro-ops), read from its text.
bool txn_value(Parser &ps, Names &names, std::vector<int64_t> &out) {
    if (!ps.prefixes()) return false;
    if (*ps.p != '[') {
        uint8_t kind;
        int64_t v;
        return ps.scalar(kind, v) && kind == K_NIL;
    }
    ++ps.p;
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return false;
        if (*ps.p == ']') { ++ps.p; return true; }
        if (!micro_op(ps, names, out)) return false;
    }
}

template <class V>
int64_t scal(const V &v, bool &ok) {
    if (v.kind == K_NIL) return LC_NIL;
    if (v.kind == K_INT) return v.i;
    ok = false;
    return LC_NIL;
}

template <class V>
bool register_value(uint8_t f, const V &val, int64_t &v0, int64_t &v1) {
    bool ok = true;
    if (f == LC_F_ACQUIRE || f == LC_F_RELEASE) return true;  // mutex ops carry no register value
    if (f == LC_F_CAS) {
        if (val.kind == K_VEC && val.n == 2) { v0 = scal(val.e[0], ok); v1 = scal(val.e[1], ok); }
        else if (val.kind != K_NIL) ok = false;
        return ok;
    }
    v0 = scal(val, ok);
    return ok;
}

// One row from a parsed op.  indep: values are [k v] tuples.  A :txn row's
// micro-ops are read from the value's text (names: the register interner).
int convert(const RawOp &o, bool indep, lc_hist &h, Names *names, const char *end, const char *base) {
    int64_t key = LC_NO_KEY, v0 = LC_NIL, v1 = LC_NIL;
    if (o.f == LC_F_TXN) {
        std::vector<int64_t> mops;
        if (o.vb) {
            Parser tp{o.vb, end, base};
            if (indep) {
                tp.ws();
                ++tp.p;  // '[' of the [k txn] tuple (txn_tuple checked it)
                uint8_t kind;
                tp.ws();
                if (!tp.scalar(kind, key) || kind != K_INT) return CONV_KEY;
            }
            if (!txn_value(tp, *names, mops)) return CONV_TXN;
        }
        h.push(o.type, o.f, o.process, key, v0, v1, o.index);
        h.set_mops(mops.data(), mops.size() / 3);
        return CONV_OK;
    }
    if (o.f == LC_F_OTHER) {
        if (o.nem >= 0) v0 = o.nem;
    } else if (indep) {
        bool ok = true;
        key = scal(o.value.e[0], ok);
        if (!ok || key == LC_NIL) return CONV_KEY;
        if (!register_value(o.f, o.value.e[1], v0, v1)) return CONV_VALUE;
    } else {
        if (!register_value(o.f, o.value, v0, v1)) return CONV_VALUE;
    }
    h.push(o.type, o.f, o.process, key, v0, v1, o.index);
    return CONV_OK;
}

// Parse [b, e) of one-op-per-line text (or, whole=true, the full text in
// either form) into rows.  Tuple mode is assumed; a client op whose value is
// not a 2-vector ends the chunk with not_indep set.
struct alignas(256) Chunk {
    lc_hist rows;
    std::string err;
    size_t err_off = 0;
    int conv_err = CONV_OK;
    int64_t conv_row = -1;  // chunk-local op number of a conversion error
    bool not_indep = false, any_client = false;
    bool need_serial = false;  // a :txn op in a parallel chunk (one interner for the whole file)
    Names names;
};

void parse_range(const char *base, const char *b, const char *e, bool indep, bool whole, Chunk &out) {
    Parser ps{b, e, base};
    out.rows.reserve((size_t)(e - b) / 64 + 16);  // ~70-100 bytes per Jepsen op line
    auto one = [&](void) -> bool {
        RawOp op;
        if (!read_op(ps, op)) return false;
        if (op.f == LC_F_TXN && !whole) { out.need_serial = true; return false; }
        if (op.f != LC_F_OTHER) {
            out.any_client = true;
            const bool tup = op.f == LC_F_TXN ? txn_tuple(op.value) : (op.value.kind == K_VEC && op.value.n == 2);
            if (indep && !tup) { out.not_indep = true; return false; }
        }
        const int rc = convert(op, indep, out.rows, &out.names, e, base);
        if (rc != CONV_OK) { out.conv_err = rc; out.conv_row = out.rows.size(); return false; }
        return true;
    };
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) break;
        if (*ps.p == '{') {
            if (!one()) break;
        } else if (whole && *ps.p == '[') {  // a vector of op maps
            ++ps.p;
            bool closed = false;
            for (;;) {
                ps.ws();
                if (ps.p >= ps.end) { ps.fail("unterminated history vector"); break; }
                if (*ps.p == ']') { ++ps.p; closed = true; break; }
                if (*ps.p != '{') { ps.fail("expected an op map"); break; }
                if (!one()) break;
            }
            if (!closed) break;
        } else {
            ps.fail("expected an op map");
            break;
        }
    }
    out.err = ps.err;
    out.err_off = ps.err_off;
}

int64_t line_of(const char *text, size_t off) {
    return 1 + (int64_t)std::count(text, text + off, '\n');
}

int finish_serial(const char *text, int64_t len, lc_hist **out) {
    // pass 1 assumes [k v] tuples; a client op that is not one means the
    // history is not independent and it is read again with plain values
    for (int pass = 0; pass < 2; ++pass) {
        const bool indep = pass == 0;
        auto *c = new (std::nothrow) Chunk();
        if (!c) return lc::fail(LC_E_NOMEM, "lc_edn: out of memory");
        parse_range(text, text, text + len, indep, true, *c);
        if (!c->err.empty()) {
            const int rc = lc::fail(LC_E_PARSE, "lc_edn: line %lld: %s", (long long)line_of(text, c->err_off),
                                    c->err.c_str());
            delete c;
            return rc;
        }
        if (indep && (c->not_indep || !c->any_client)) { delete c; continue; }
        if (c->conv_err != CONV_OK) {
            const int rc = c->conv_err == CONV_KEY
                               ? lc::fail(LC_E_UNSUPPORTED, "lc_edn: op %lld: tuple key is not an integer",
                                          (long long)c->conv_row)
                           : c->conv_err == CONV_TXN
                               ? lc::fail(LC_E_UNSUPPORTED,
                                          "lc_edn: op %lld: :txn value is not nil or [[:read|:write k v] ...]",
                                          (long long)c->conv_row)
                               : lc::fail(LC_E_UNSUPPORTED,
                                          "lc_edn: op %lld: value is not an integer, nil or [old new]",
                                          (long long)c->conv_row);
            delete c;
            return rc;
        }
        lc_hist *h = new (std::nothrow) lc_hist(std::move(c->rows));
        if (h) {
            h->reg_names = std::move(c->names.names);
            h->finish_mops();
        }
        delete c;
        if (!h) return lc::fail(LC_E_NOMEM, "lc_edn: out of memory");
        *out = h;
        return LC_OK;
    }
    return lc::fail(LC_E_PARSE, "lc_edn: internal error");  // not reached
}

}  // namespace

extern "C" int lc_edn_parse(const char *text, int64_t len, lc_hist **out) {
    lc::Range range("lc_edn_parse");
    if (!text || !out || len < 0) return lc::fail(LC_E_INVALID, "lc_edn_parse: null argument");
    try {
        const char *b = text, *e = text + len;
        while (b < e && (*b == ' ' || *b == '\n' || *b == '\t' || *b == '\r' || *b == ',')) ++b;
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        int T = (int)std::min<int64_t>({16, (int64_t)hw, len >> 20});
        if (const char *ev = std::getenv("LC_EDN_THREADS")) T = std::min(T, std::atoi(ev));
        if (T < 2 || b >= e || *b != '{') return finish_serial(text, len, out);
        // split at line starts that open an op map
        std::vector<const char *> cut{b};
        for (int i = 1; i < T; ++i) {
            const char *q = std::max(cut.back(), text + len * i / T);
            while (q < e && !(q[-1] == '\n' && *q == '{')) ++q;
            if (q < e && q > cut.back()) cut.push_back(q);
        }
        cut.push_back(e);
        const size_t n = cut.size() - 1;
        std::vector<Chunk> ch(n);
        std::vector<std::thread> th;
        th.reserve(n);
        bool spawned = true;
        try {
            for (size_t i = 0; i < n; ++i)
                th.emplace_back([&, i] { parse_range(text, cut[i], cut[i + 1], true, false, ch[i]); });
        } catch (const std::system_error &) {
            spawned = false;  // joined below, then the serial read
        }
        for (auto &t : th) t.join();
        if (!spawned) return finish_serial(text, len, out);
        bool any_client = false;
        for (auto &c : ch) {
            if (!c.err.empty() || c.not_indep || c.need_serial || c.conv_err != CONV_OK) return finish_serial(text, len, out);
            any_client |= c.any_client;
        }
        if (!any_client) return finish_serial(text, len, out);
        lc_hist *h = new (std::nothrow) lc_hist();
        if (!h) return lc::fail(LC_E_NOMEM, "lc_edn: out of memory");
        size_t total = 0;
        for (auto &c : ch) total += c.rows.type.size();
        h->reserve(total);
        for (auto &c : ch) {
            auto app = [](auto &dst, auto &src) { dst.insert(dst.end(), src.begin(), src.end()); };
            app(h->type, c.rows.type); app(h->f, c.rows.f); app(h->process, c.rows.process);
            app(h->key, c.rows.key); app(h->v0, c.rows.v0); app(h->v1, c.rows.v1); app(h->index, c.rows.index);
            c.rows = lc_hist();
        }
        *out = h;
        return LC_OK;
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_edn: out of memory");
    } catch (const std::system_error &) {
        return finish_serial(text, len, out);  // no threads: serial read
    }
}

extern "C" int lc_edn_read(const char *path, lc_hist **out) {
    if (!path || !out) return lc::fail(LC_E_INVALID, "lc_edn_read: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_read: cannot open %s", path);
    std::string s;
    try {
        if (std::fseek(f, 0, SEEK_END) == 0) {
            const long sz = std::ftell(f);
            if (sz > 0) s.resize((size_t)sz);
            std::rewind(f);
        }
        size_t got = s.empty() ? 0 : std::fread(&s[0], 1, s.size(), f);
        s.resize(got);
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, r);  // growing / unseekable files
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return lc::fail(LC_E_NOMEM, "lc_edn_read: out of memory");
    }
    std::fclose(f);
    return lc_edn_parse(s.data(), (int64_t)s.size(), out);
}

static void put_scalar(std::string &o, int64_t v) {
    if (v == LC_NIL) o += "nil"; else o += std::to_string(v);
}

// A register name as lc_edn_read keeps it (":x", "\"z\"", ...) is written back
// verbatim when it reads as one EDN token; anything else becomes :r<i>.
static bool edn_token(const char *s) {
    if (!s || !*s) return false;
    if (*s == '"') {
        const size_t n = std::strlen(s);
        if (n < 2 || s[n - 1] != '"') return false;
        for (size_t i = 1; i + 1 < n; ++i)
            if (s[i] == '"' || s[i] == '\\' || s[i] == '\n') return false;
        return true;
    }
    for (const char *c = s; *c; ++c)
        if (std::isspace((unsigned char)*c) || std::strchr("[](){}\",;\\", *c)) return false;
    return true;
}

extern "C" int lc_edn_write(const char *path, const lc_history *h) { return lc_edn_write_named(path, h, nullptr, 0); }

extern "C" int lc_edn_write_named(const char *path, const lc_history *h, const char *const *reg_names,
                                  int64_t n_reg_names) {
    if (!path || !h || h->n < 0) return lc::fail(LC_E_INVALID, "lc_edn_write: null argument");
    if (n_reg_names < 0 || (n_reg_names > 0 && !reg_names))
        return lc::fail(LC_E_INVALID, "lc_edn_write_named: bad register names");
    FILE *f = std::fopen(path, "wb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_write: cannot open %s", path);
    static const char *types[] = {"invoke", "ok", "fail", "info"};
    static const char *fs[] = {"read", "write", "cas", "", "acquire", "release", "txn"};
    std::string line;
    for (int64_t r = 0; r < h->n; ++r) {
        line.clear();
        if (h->type[r] > LC_INFO || h->f[r] > LC_F_TXN) { std::fclose(f); return lc::fail(LC_E_INVALID, "lc_edn_write: bad row %lld", (long long)r); }
        line += "{:type :"; line += types[h->type[r]];
        if (h->f[r] == LC_F_TXN) {
            // [[:read k v] ...]; named registers (ids from LC_NAMED_REG_BASE) by
            // their names when given, else as :r<i>
            std::string v = "nil";
            const int64_t mb = h->mop_off ? h->mop_off[r] : 0, me = h->mop_off ? h->mop_off[r + 1] : 0;
            if (me > mb) {
                v = "[";
                for (int64_t m = mb; m < me; ++m) {
                    const int64_t *t = h->mop + 3 * m;
                    v += m > mb ? " [:" : "[:";
                    v += t[0] == LC_MOP_WRITE ? "write " : "read ";
                    const int64_t ni = t[1] - LC_NAMED_REG_BASE;
                    if (t[1] >= LC_NAMED_REG_BASE && ni < n_reg_names && edn_token(reg_names[ni])) v += reg_names[ni];
                    else if (t[1] >= LC_NAMED_REG_BASE) { v += ":r"; v += std::to_string(ni); }
                    else v += std::to_string(t[1]);
                    v += " ";
                    put_scalar(v, t[2]);
                    v += "]";
                }
                v += "]";
            }
            line += ", :f :txn, :value ";
            if (h->key[r] != LC_NO_KEY) { line += "["; line += std::to_string(h->key[r]); line += " "; line += v; line += "]"; }
            else line += v;
        } else if (h->f[r] == LC_F_OTHER) {
            line += ", :f :"; line += h->v0[r] == 1 ? "start" : h->v0[r] == 0 ? "stop" : "nemesis";
            line += ", :value nil";
        } else {
            line += ", :f :"; line += fs[h->f[r]];
            line += ", :value ";
            std::string v;
            if (h->f[r] == LC_F_ACQUIRE || h->f[r] == LC_F_RELEASE) {
                v = "nil";
            } else if (h->f[r] == LC_F_CAS) {
                if (h->v0[r] == LC_NIL && h->v1[r] == LC_NIL && h->type[r] == LC_INVOKE) v = "nil";
                else { v = "["; put_scalar(v, h->v0[r]); v += " "; put_scalar(v, h->v1[r]); v += "]"; }
            } else {
                put_scalar(v, h->v0[r]);
            }
            if (h->key[r] != LC_NO_KEY) { line += "["; line += std::to_string(h->key[r]); line += " "; line += v; line += "]"; }
            else line += v;
        }
        line += ", :process ";
        if (h->process[r] == LC_NO_PROCESS) line += ":nemesis"; else line += std::to_string(h->process[r]);
        line += ", :index ";
        line += std::to_string(h->index && h->index[r] >= 0 ? h->index[r] : r);
        line += "}\n";
        if (std::fwrite(line.data(), 1, line.size(), f) != line.size()) { std::fclose(f); return lc::fail(LC_E_IO, "lc_edn_write: write failed"); }
    }
    if (std::fclose(f) != 0) return lc::fail(LC_E_IO, "lc_edn_write: close failed");
    return LC_OK;
}

// ---- the set workload's history.edn (set.clj:25-35; ABI 12) -------------------
// A second op handler over the same reader: :f :add / :read are the client
// ops, an add's :value is an integer, a read's nil or a #{...} / [...] / (...)
// of integers, either optionally inside an independent tuple [k v].  Tuples
// are decided per history as above: every client op's value is a 2-vector
// whose first element is an integer (and, for a read, whose second is not --
// a plain read [1 2] of two elements is no tuple).  Single-threaded.

struct lc_set_hist {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> key, elem, read_off, read_elem, index;
};

namespace {

struct SetRaw {
    uint8_t type = 255, f = LC_SF_OTHER;
    int64_t index = -1;
    const char *vb = nullptr;  // the :value's text
};

bool read_set_op(Parser &ps, SetRaw &op) {
    ++ps.p;  // at '{'
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated op map");
        if (*ps.p == '}') { ++ps.p; break; }
        std::string_view k;
        bool is_kw = false;
        if (!ps.keyword(k, is_kw)) return false;
        if (!is_kw) {
            if (!ps.skip()) return false;
            continue;
        }
        const Field fld = field_of(k);
        if (fld == FLD_TYPE || fld == FLD_F) {
            std::string_view v;
            bool vk = false;
            if (!ps.keyword(v, vk)) return false;
            if (fld == FLD_TYPE) {
                if (!vk) return ps.fail(":type is not a keyword");
                switch (pack8(v)) {
                    case P8("invoke"): op.type = LC_INVOKE; break;
                    case P8("ok"): op.type = LC_OK_T; break;
                    case P8("fail"): op.type = LC_FAIL; break;
                    case P8("info"): op.type = LC_INFO; break;
                    default: return ps.fail("unknown :type :" + std::string(v));
                }
            } else {
                op.f = !vk ? LC_SF_OTHER : pack8(v) == P8("add") ? LC_SF_ADD : pack8(v) == P8("read") ? LC_SF_READ : LC_SF_OTHER;
            }
        } else if (fld == FLD_INDEX) {
            Leaf v;
            if (!ps.shaped(v)) return false;
            op.index = v.kind == K_INT ? v.i : -1;
        } else if (fld == FLD_VALUE) {
            if (!ps.prefixes()) return false;
            op.vb = ps.p;
            if (!ps.skip()) return false;
        } else {
            if (!ps.skip()) return false;
        }
    }
    if (op.type == 255) return ps.fail("op map without :type");
    return true;
}

// One element (or an add's value): an integer, else LC_NIL with the value skipped.
bool set_element(Parser &ps, int64_t &out) {
    out = LC_NIL;
    if (!ps.prefixes()) return false;
    const char c = *ps.p;
    if (c == '[' || c == '(' || c == '{' || c == '"' || c == '\\' || c == ':' || c == '#') return ps.skip();
    uint8_t kind;
    int64_t v = 0;
    if (!ps.scalar(kind, v)) return false;
    if (kind == K_INT) out = v;
    return true;
}

// A read's value from its text: nil (*is_nil), or a collection whose
// elements are appended to out; anything else reads as one bad element.
bool set_read_value(Parser &ps, bool &is_nil, std::vector<int64_t> &out) {
    is_nil = false;
    if (!ps.prefixes()) return false;
    char close = 0;
    if (*ps.p == '[') { close = ']'; ++ps.p; }
    else if (*ps.p == '(') { close = ')'; ++ps.p; }
    else if (*ps.p == '#' && ps.p + 1 < ps.end && ps.p[1] == '{') { close = '}'; ps.p += 2; }
    if (!close) {
        int64_t v;
        const char *b = ps.p;
        if (!set_element(ps, v)) return false;
        if (std::string_view(b, (size_t)(ps.p - b)) == "nil") is_nil = true;
        else out.push_back(LC_NIL);
        return true;
    }
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated collection");
        if (*ps.p == close) { ++ps.p; return true; }
        int64_t v;
        if (!set_element(ps, v)) return false;
        out.push_back(v);
    }
}

int parse_set(const char *text, int64_t len, lc_set_hist **out) {
    Parser ps{text, text + len, text};
    std::vector<SetRaw> ops;
    auto one = [&]() -> bool {
        SetRaw op;
        if (!read_set_op(ps, op)) return false;
        ops.push_back(op);
        return true;
    };
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) break;
        if (*ps.p == '{') {
            if (!one()) break;
        } else if (*ps.p == '[') {  // a vector of op maps
            ++ps.p;
            bool closed = false;
            for (;;) {
                ps.ws();
                if (ps.p >= ps.end) { ps.fail("unterminated history vector"); break; }
                if (*ps.p == ']') { ++ps.p; closed = true; break; }
                if (*ps.p != '{') { ps.fail("expected an op map"); break; }
                if (!one()) break;
            }
            if (!closed) break;
        } else {
            ps.fail("expected an op map");
            break;
        }
    }
    if (!ps.err.empty())
        return lc::fail(LC_E_PARSE, "lc_edn_set: line %lld: %s", (long long)line_of(text, ps.err_off), ps.err.c_str());
    // tuples?
    bool indep = false, any_client = false;
    for (const SetRaw &o : ops) {
        if (o.f == LC_SF_OTHER) continue;
        bool tup = false;
        if (o.vb) {
            Parser vp{o.vb, text + len, text};
            Top v;
            if (vp.shaped(v))
                tup = v.kind == K_VEC && v.n == 2 && v.e[0].kind == K_INT && (o.f == LC_SF_ADD || v.e[1].kind != K_INT);
        }
        indep = any_client ? indep && tup : tup;
        any_client = true;
    }
    auto *h = new lc_set_hist();
    h->read_off.push_back(0);
    for (size_t r = 0; r < ops.size(); ++r) {
        const SetRaw &o = ops[r];
        int64_t key = LC_NO_KEY, elem = 0;
        if (o.f != LC_SF_OTHER) {
            Parser vp{o.vb ? o.vb : "nil", o.vb ? text + len : nullptr, text};
            if (!o.vb) vp.end = vp.p + 3;
            bool ok = true;
            if (indep) {
                vp.ws();
                ++vp.p;  // '[' of the tuple (checked above)
                vp.ws();
                uint8_t kind;
                ok = vp.scalar(kind, key) && kind == K_INT;
            }
            if (ok && o.f == LC_SF_ADD) {
                ok = set_element(vp, elem);
            } else if (ok) {
                bool is_nil = false;
                ok = set_read_value(vp, is_nil, h->read_elem);
                elem = is_nil ? LC_NIL : 0;
            }
            if (!ok) {
                delete h;
                return lc::fail(LC_E_PARSE, "lc_edn_set: op %lld: %s", (long long)r, vp.err.empty() ? "bad :value" : vp.err.c_str());
            }
        }
        h->type.push_back(o.type); h->f.push_back(o.f); h->key.push_back(key); h->elem.push_back(elem);
        h->index.push_back(o.index);
        h->read_off.push_back((int64_t)h->read_elem.size());
    }
    *out = h;
    return LC_OK;
}

}  // namespace

extern "C" int lc_edn_parse_set(const char *text, int64_t len, lc_set_hist **out) {
    lc::Range range("lc_edn_parse_set");
    if (!text || !out || len < 0) return lc::fail(LC_E_INVALID, "lc_edn_parse_set: null argument");
    try {
        return parse_set(text, len, out);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_edn_set: out of memory");
    }
}

extern "C" int lc_edn_read_set(const char *path, lc_set_hist **out) {
    if (!path || !out) return lc::fail(LC_E_INVALID, "lc_edn_read_set: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_read_set: cannot open %s", path);
    std::string s;
    try {
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, r);
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return lc::fail(LC_E_NOMEM, "lc_edn_read_set: out of memory");
    }
    std::fclose(f);
    return lc_edn_parse_set(s.data(), (int64_t)s.size(), out);
}

extern "C" int lc_set_hist_view(const lc_set_hist *h, lc_set_history *out) {
    if (!h || !out) return lc::fail(LC_E_INVALID, "lc_set_hist_view: null argument");
    out->n = (int64_t)h->type.size();
    out->type = h->type.data(); out->f = h->f.data(); out->key = h->key.data(); out->elem = h->elem.data();
    out->read_off = h->read_off.data(); out->read_elem = h->read_elem.data(); out->index = h->index.data();
    return LC_OK;
}

extern "C" void lc_set_hist_free(lc_set_hist *h) { delete h; }

// ---- history.edn for checker/perf (ABI 13) -------------------------------------
// A third op handler over the same reader: :type, :f, :process and :time of
// every op map, every :value skipped.  :f names (any keyword; another kind of
// value reads as its text) are interned in order of first appearance; an op
// map without :f gets the name "nil".  A map without an integer :time is a
// parse error: no latency can be computed from it.  Single-threaded.

struct lc_perf_hist {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> process, time;
    std::vector<std::string> names;
};

namespace {

struct PerfNames {
    std::unordered_map<std::string, uint32_t> id;
    std::vector<std::string> *names;
    std::string_view last;  // the last name looked up (most ops repeat it)
    uint32_t last_id = 0;
    uint32_t of(std::string_view t) {
        if (!last.empty() && t == last) return last_id;
        auto it = id.find(std::string(t));
        if (it == id.end()) {
            names->emplace_back(t);
            it = id.emplace(names->back(), (uint32_t)names->size() - 1).first;
        }
        last = it->first;
        last_id = it->second;
        return last_id;
    }
};

bool read_perf_op(Parser &ps, PerfNames &names, lc_perf_hist &h) {
    ++ps.p;  // at '{'
    uint8_t type = 255;
    int64_t process = LC_NO_PROCESS, time = 0;
    bool have_time = false;
    std::string_view fname = "nil";
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated op map");
        if (*ps.p == '}') { ++ps.p; break; }
        std::string_view k;
        bool is_kw = false;
        if (!ps.keyword(k, is_kw)) return false;
        if (!is_kw) {
            if (!ps.skip()) return false;
            continue;
        }
        const uint64_t k8 = pack8(k);
        if (k8 == P8("type")) {
            std::string_view v;
            bool vk = false;
            if (!ps.keyword(v, vk)) return false;
            if (!vk) return ps.fail(":type is not a keyword");
            switch (pack8(v)) {
                case P8("invoke"): type = LC_INVOKE; break;
                case P8("ok"): type = LC_OK_T; break;
                case P8("fail"): type = LC_FAIL; break;
                case P8("info"): type = LC_INFO; break;
                default: return ps.fail("unknown :type :" + std::string(v));
            }
        } else if (k8 == P8("f")) {
            if (!ps.prefixes()) return false;
            const char *b = ps.p;
            if (*ps.p == ':') {
                bool vk = false;
                if (!ps.keyword(fname, vk)) return false;
            } else {
                if (!ps.skip()) return false;
                fname = std::string_view(b, (size_t)(ps.p - b));
            }
        } else if (k8 == P8("process") || k8 == P8("time")) {
            Leaf v;
            if (!ps.shaped(v)) return false;
            if (k8 == P8("process")) {
                process = v.kind == K_INT ? v.i : LC_NO_PROCESS;
            } else {
                if (v.kind != K_INT) return ps.fail(":time is not an integer");
                time = v.i;
                have_time = true;
            }
        } else {
            if (!ps.skip()) return false;
        }
    }
    if (type == 255) return ps.fail("op map without :type");
    if (!have_time) return ps.fail("op map without :time");
    const uint32_t f = names.of(fname);
    if (f > 255) return ps.fail("more than 256 distinct :f");
    h.type.push_back(type); h.f.push_back((uint8_t)f); h.process.push_back(process); h.time.push_back(time);
    return true;
}

int parse_perf(const char *text, int64_t len, lc_perf_hist **out) {
    Parser ps{text, text + len, text};
    auto *h = new lc_perf_hist();
    PerfNames names;
    names.names = &h->names;
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) break;
        if (*ps.p == '{') {
            if (!read_perf_op(ps, names, *h)) break;
        } else if (*ps.p == '[') {  // a vector of op maps
            ++ps.p;
            bool closed = false;
            for (;;) {
                ps.ws();
                if (ps.p >= ps.end) { ps.fail("unterminated history vector"); break; }
                if (*ps.p == ']') { ++ps.p; closed = true; break; }
                if (*ps.p != '{') { ps.fail("expected an op map"); break; }
                if (!read_perf_op(ps, names, *h)) break;
            }
            if (!closed) break;
        } else {
            ps.fail("expected an op map");
            break;
        }
    }
    if (!ps.err.empty()) {
        delete h;
        return lc::fail(LC_E_PARSE, "lc_edn_perf: line %lld: %s", (long long)line_of(text, ps.err_off), ps.err.c_str());
    }
    *out = h;
    return LC_OK;
}

}  // namespace

extern "C" int lc_edn_parse_perf(const char *text, int64_t len, lc_perf_hist **out) {
    lc::Range range("lc_edn_parse_perf");
    if (!text || !out || len < 0) return lc::fail(LC_E_INVALID, "lc_edn_parse_perf: null argument");
    try {
        return parse_perf(text, len, out);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_edn_perf: out of memory");
    }
}

extern "C" int lc_edn_read_perf(const char *path, lc_perf_hist **out) {
    if (!path || !out) return lc::fail(LC_E_INVALID, "lc_edn_read_perf: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_read_perf: cannot open %s", path);
    std::string s;
    try {
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, r);
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return lc::fail(LC_E_NOMEM, "lc_edn_read_perf: out of memory");
    }
    std::fclose(f);
    return lc_edn_parse_perf(s.data(), (int64_t)s.size(), out);
}

extern "C" int lc_perf_hist_view(const lc_perf_hist *h, lc_perf_history *out) {
    if (!h || !out) return lc::fail(LC_E_INVALID, "lc_perf_hist_view: null argument");
    out->n = (int64_t)h->type.size();
    out->type = h->type.data(); out->f = h->f.data(); out->process = h->process.data(); out->time = h->time.data();
    out->n_f = (int32_t)h->names.size();
    out->f_start = out->f_stop = -1;
    for (size_t i = 0; i < h->names.size(); ++i) {
        if (h->names[i] == "start") out->f_start = (int32_t)i;
        if (h->names[i] == "stop") out->f_stop = (int32_t)i;
    }
    return LC_OK;
}

extern "C" const char *lc_perf_hist_name(const lc_perf_hist *h, int64_t i) {
    if (!h || i < 0 || (size_t)i >= h->names.size()) return nullptr;
    return h->names[(size_t)i].c_str();
}

extern "C" void lc_perf_hist_free(lc_perf_hist *h) { delete h; }

// ---- history.edn for checker/set-full (ABI 13, additive) -------------------------
// The set reader's op handler decides everything it decides for lc_edn_read_set
// (parse_set above: client ops, tuples, elements); a second walk over the same
// text with the reader keeps every op map's :process (LC_NO_PROCESS when it is
// no integer) and :time (0 when absent or no integer).  Single-threaded.

struct lc_setfull_hist {
    lc_set_hist *base = nullptr;
    std::vector<int64_t> process, time;
    ~lc_setfull_hist() { delete base; }
};

namespace {

bool read_setfull_meta(Parser &ps, lc_setfull_hist &h) {
    ++ps.p;  // at '{'
    int64_t process = LC_NO_PROCESS, time = 0;
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated op map");
        if (*ps.p == '}') { ++ps.p; break; }
        std::string_view k;
        bool is_kw = false;
        if (!ps.keyword(k, is_kw)) return false;
        const uint64_t k8 = is_kw ? pack8(k) : 0;
        if (is_kw && (k8 == P8("process") || k8 == P8("time"))) {
            Leaf v;
            if (!ps.shaped(v)) return false;
            if (k8 == P8("process")) process = v.kind == K_INT ? v.i : LC_NO_PROCESS;
            else time = v.kind == K_INT ? v.i : 0;
        } else {
            if (!ps.skip()) return false;
        }
    }
    h.process.push_back(process);
    h.time.push_back(time);
    return true;
}

int parse_setfull(const char *text, int64_t len, lc_setfull_hist **out) {
    auto h = std::make_unique<lc_setfull_hist>();
    if (int rc = parse_set(text, len, &h->base)) return rc;
    Parser ps{text, text + len, text};
    for (;;) {  // the text parsed once already: op maps, bare or in one vector
        ps.ws();
        if (ps.p >= ps.end) break;
        if (*ps.p == '[' || *ps.p == ']') { ++ps.p; continue; }
        if (*ps.p != '{' || !read_setfull_meta(ps, *h)) break;
    }
    if (!ps.err.empty() || h->process.size() != h->base->type.size())
        return lc::fail(LC_E_PARSE, "lc_edn_setfull: line %lld: %s", (long long)line_of(text, ps.err_off),
                        ps.err.empty() ? "op maps differ between the two walks" : ps.err.c_str());
    *out = h.release();
    return LC_OK;
}

}  // namespace

extern "C" int lc_edn_parse_setfull(const char *text, int64_t len, lc_setfull_hist **out) {
    lc::Range range("lc_edn_parse_setfull");
    if (!text || !out || len < 0) return lc::fail(LC_E_INVALID, "lc_edn_parse_setfull: null argument");
    try {
        return parse_setfull(text, len, out);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_edn_setfull: out of memory");
    }
}

extern "C" int lc_edn_read_setfull(const char *path, lc_setfull_hist **out) {
    if (!path || !out) return lc::fail(LC_E_INVALID, "lc_edn_read_setfull: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_read_setfull: cannot open %s", path);
    std::string s;
    try {
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, r);
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return lc::fail(LC_E_NOMEM, "lc_edn_read_setfull: out of memory");
    }
    std::fclose(f);
    return lc_edn_parse_setfull(s.data(), (int64_t)s.size(), out);
}

extern "C" int lc_setfull_hist_view(const lc_setfull_hist *h, lc_setfull_history *out) {
    if (!h || !out) return lc::fail(LC_E_INVALID, "lc_setfull_hist_view: null argument");
    const lc_set_hist *b = h->base;
    out->n = (int64_t)b->type.size();
    out->type = b->type.data(); out->f = b->f.data(); out->key = b->key.data(); out->elem = b->elem.data();
    out->read_off = b->read_off.data(); out->read_elem = b->read_elem.data(); out->index = b->index.data();
    out->process = h->process.data(); out->time = h->time.data();
    return LC_OK;
}

extern "C" void lc_setfull_hist_free(lc_setfull_hist *h) { delete h; }

// ---- history.edn for checker/counter (include/lincheck_counter.h) ----------------
// A fourth op handler over the same reader: :type, :f (:add / :read, anything
// else LC_CF_OTHER), :process, :index and the :value, which is an integer or
// nil, or either inside an independent tuple [k v] -- a two-element vector
// whose first element is an integer.  Any other value reads as LC_NIL.
// Single-threaded.

#include "../../include/lincheck_counter.h"

struct lc_counter_hist {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> process, key, value, index;
};

namespace {

bool read_counter_op(Parser &ps, lc_counter_hist &h) {
    ++ps.p;  // at '{'
    uint8_t type = 255, f = LC_CF_OTHER;
    int64_t process = LC_NO_PROCESS, index = -1;
    Top value;
    value.kind = K_NIL;
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated op map");
        if (*ps.p == '}') { ++ps.p; break; }
        std::string_view k;
        bool is_kw = false;
        if (!ps.keyword(k, is_kw)) return false;
        if (!is_kw) {
            if (!ps.skip()) return false;
            continue;
        }
        const Field fld = field_of(k);
        if (fld == FLD_TYPE || fld == FLD_F) {
            std::string_view v;
            bool vk = false;
            if (!ps.keyword(v, vk)) return false;
            if (fld == FLD_TYPE) {
                if (!vk) return ps.fail(":type is not a keyword");
                switch (pack8(v)) {
                    case P8("invoke"): type = LC_INVOKE; break;
                    case P8("ok"): type = LC_OK_T; break;
                    case P8("fail"): type = LC_FAIL; break;
                    case P8("info"): type = LC_INFO; break;
                    default: return ps.fail("unknown :type :" + std::string(v));
                }
            } else {
                f = !vk ? LC_CF_OTHER : pack8(v) == P8("add") ? LC_CF_ADD : pack8(v) == P8("read") ? LC_CF_READ : LC_CF_OTHER;
            }
        } else if (fld == FLD_PROCESS || fld == FLD_INDEX) {
            Leaf v;
            if (!ps.shaped(v)) return false;
            if (fld == FLD_PROCESS) process = v.kind == K_INT ? v.i : LC_NO_PROCESS;
            else index = v.kind == K_INT ? v.i : -1;
        } else if (fld == FLD_VALUE) {
            if (!ps.shaped(value)) return false;
        } else {
            if (!ps.skip()) return false;
        }
    }
    if (type == 255) return ps.fail("op map without :type");
    int64_t key = LC_NO_KEY, v = LC_NIL;
    if (f != LC_CF_OTHER) {
        if (value.kind == K_VEC && value.n == 2 && value.e[0].kind == K_INT) {
            key = value.e[0].i;
            if (value.e[1].kind == K_INT) v = value.e[1].i;
        } else if (value.kind == K_INT) {
            v = value.i;
        }
    }
    h.type.push_back(type); h.f.push_back(f); h.process.push_back(process); h.key.push_back(key);
    h.value.push_back(v); h.index.push_back(index);
    return true;
}

int parse_counter(const char *text, int64_t len, lc_counter_hist **out) {
    Parser ps{text, text + len, text};
    auto h = std::make_unique<lc_counter_hist>();
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) break;
        if (*ps.p == '{') {
            if (!read_counter_op(ps, *h)) break;
        } else if (*ps.p == '[') {  // a vector of op maps
            ++ps.p;
            bool closed = false;
            for (;;) {
                ps.ws();
                if (ps.p >= ps.end) { ps.fail("unterminated history vector"); break; }
                if (*ps.p == ']') { ++ps.p; closed = true; break; }
                if (*ps.p != '{') { ps.fail("expected an op map"); break; }
                if (!read_counter_op(ps, *h)) break;
            }
            if (!closed) break;
        } else {
            ps.fail("expected an op map");
            break;
        }
    }
    if (!ps.err.empty())
        return lc::fail(LC_E_PARSE, "lc_edn_counter: line %lld: %s", (long long)line_of(text, ps.err_off), ps.err.c_str());
    *out = h.release();
    return LC_OK;
}

}  // namespace

extern "C" int lc_edn_parse_counter(const char *text, int64_t len, lc_counter_hist **out) {
    lc::Range range("lc_edn_parse_counter");
    if (!text || !out || len < 0) return lc::fail(LC_E_INVALID, "lc_edn_parse_counter: null argument");
    try {
        return parse_counter(text, len, out);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_edn_counter: out of memory");
    }
}

extern "C" int lc_edn_read_counter(const char *path, lc_counter_hist **out) {
    if (!path || !out) return lc::fail(LC_E_INVALID, "lc_edn_read_counter: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_read_counter: cannot open %s", path);
    std::string s;
    try {
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, r);
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return lc::fail(LC_E_NOMEM, "lc_edn_read_counter: out of memory");
    }
    std::fclose(f);
    return lc_edn_parse_counter(s.data(), (int64_t)s.size(), out);
}

extern "C" int lc_counter_hist_view(const lc_counter_hist *h, lc_counter_history *out) {
    if (!h || !out) return lc::fail(LC_E_INVALID, "lc_counter_hist_view: null argument");
    out->n = (int64_t)h->type.size();
    out->type = h->type.data(); out->f = h->f.data(); out->process = h->process.data(); out->key = h->key.data();
    out->value = h->value.data(); out->index = h->index.data();
    return LC_OK;
}

extern "C" void lc_counter_hist_free(lc_counter_hist *h) { delete h; }

// ---- history.edn for checker/total-queue and /unique-ids (include/lincheck_queue.h) ----
// A fifth op handler over the same reader: :type, :f (:enqueue / :dequeue /
// :drain / :generate, anything else LC_QF_OTHER) and the :value.  The value's
// text is skipped where it stands and read again once the op's :f is known: an
// integer or nil, a drain's vector of them, or either inside an independent
// tuple [k v].  A value of any other shape ends the read with
// LC_E_UNSUPPORTED.  Single-threaded.

#include "../../include/lincheck_queue.h"

struct lc_queue_hist {
    std::vector<uint8_t> type, f;
    std::vector<int64_t> key, value, drain_val;
    std::vector<uint64_t> drain_off{0};
    // one value's elements while it is read: kinds (K_VEC: an integer vector, kept in inner) and integers
    std::vector<uint8_t> ek;
    std::vector<int64_t> ei, inner;
};

namespace {

// The elements of the vector at ps.p ('[' taken) up to its ']': integers and
// nils into ints; anything else makes `plain` false (and is skipped).
bool read_int_vector(Parser &ps, std::vector<int64_t> &ints, bool &plain) {
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated collection");
        if (*ps.p == ']') { ++ps.p; return true; }
        Leaf e;
        if (!ps.shaped(e)) return false;
        if (e.kind == K_INT) ints.push_back(e.i);
        else if (e.kind == K_NIL) ints.push_back(LC_NIL);
        else plain = false;
    }
}

// The :value at ps.p of an op whose :f is f.  shape_ok comes back false for a
// value the rules have no reading of.
bool read_queue_value(Parser &ps, uint8_t f, lc_queue_hist &h, int64_t &key, int64_t &v, bool &shape_ok) {
    key = LC_NO_KEY;
    v = LC_NIL;
    shape_ok = true;
    if (!ps.prefixes()) return false;
    const bool drain = f == LC_QF_DRAIN;
    if (*ps.p != '[') {
        Leaf s;
        if (!ps.shaped(s)) return false;
        if (s.kind == K_INT && !drain) v = s.i;
        else if (s.kind != K_NIL) shape_ok = false;
        return true;
    }
    ++ps.p;
    h.ek.clear(); h.ei.clear(); h.inner.clear();
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated collection");
        if (*ps.p == ']') { ++ps.p; break; }
        if (!ps.prefixes()) return false;
        if (*ps.p == '[') {
            ++ps.p;
            bool plain = h.ek.size() == 1 && drain;  // only a tuple's second element may be a vector
            h.inner.clear();
            if (!read_int_vector(ps, h.inner, plain)) return false;
            h.ek.push_back(plain ? K_VEC : K_OTHER);
            h.ei.push_back(0);
        } else {
            Leaf e;
            if (!ps.shaped(e)) return false;
            h.ek.push_back(e.kind);
            h.ei.push_back(e.kind == K_INT ? e.i : LC_NIL);
        }
    }
    const size_t n = h.ek.size();
    if (n == 2 && h.ek[0] == K_INT && (drain ? h.ek[1] == K_NIL || h.ek[1] == K_VEC : h.ek[1] == K_INT || h.ek[1] == K_NIL)) {
        key = h.ei[0];
        if (!drain) v = h.ei[1];
        else if (h.ek[1] == K_VEC) h.drain_val.insert(h.drain_val.end(), h.inner.begin(), h.inner.end());
        return true;
    }
    if (!drain) { shape_ok = false; return true; }
    for (size_t i = 0; i < n; ++i)
        if (h.ek[i] != K_INT && h.ek[i] != K_NIL) { shape_ok = false; return true; }
    h.drain_val.insert(h.drain_val.end(), h.ei.begin(), h.ei.end());
    return true;
}

bool read_queue_op(Parser &ps, lc_queue_hist &h, bool &unsupported) {
    ++ps.p;  // at '{'
    uint8_t type = 255, f = LC_QF_OTHER;
    const char *vb = nullptr;
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) return ps.fail("unterminated op map");
        if (*ps.p == '}') { ++ps.p; break; }
        std::string_view k;
        bool is_kw = false;
        if (!ps.keyword(k, is_kw)) return false;
        if (!is_kw) {
            if (!ps.skip()) return false;
            continue;
        }
        const Field fld = field_of(k);
        if (fld == FLD_TYPE || fld == FLD_F) {
            std::string_view v;
            bool vk = false;
            if (!ps.keyword(v, vk)) return false;
            if (fld == FLD_TYPE) {
                if (!vk) return ps.fail(":type is not a keyword");
                switch (pack8(v)) {
                    case P8("invoke"): type = LC_INVOKE; break;
                    case P8("ok"): type = LC_OK_T; break;
                    case P8("fail"): type = LC_FAIL; break;
                    case P8("info"): type = LC_INFO; break;
                    default: return ps.fail("unknown :type :" + std::string(v));
                }
            } else if (vk) {
                switch (pack8(v)) {
                    case P8("enqueue"): f = LC_QF_ENQUEUE; break;
                    case P8("dequeue"): f = LC_QF_DEQUEUE; break;
                    case P8("drain"): f = LC_QF_DRAIN; break;
                    case P8("generate"): f = LC_QF_GENERATE; break;
                    default: f = LC_QF_OTHER;
                }
            }
        } else if (fld == FLD_VALUE) {
            ps.ws();
            vb = ps.p;
            if (!ps.skip()) return false;
        } else {
            if (!ps.skip()) return false;
        }
    }
    if (type == 255) return ps.fail("op map without :type");
    int64_t key = LC_NO_KEY, v = LC_NIL;
    if (f != LC_QF_OTHER && vb) {
        Parser q{vb, ps.end, ps.base};
        bool shape_ok = true;
        if (!read_queue_value(q, f, h, key, v, shape_ok)) {
            ps.p = q.p;
            return ps.fail(q.err);
        }
        if (!shape_ok) {
            unsupported = true;
            ps.p = vb;
            return ps.fail(f == LC_QF_DRAIN ? "a :drain's value is neither nil nor a vector of integers"
                                            : "a value that is neither an integer nor nil");
        }
    }
    h.type.push_back(type); h.f.push_back(f); h.key.push_back(key); h.value.push_back(v);
    h.drain_off.push_back(h.drain_val.size());
    return true;
}

int parse_queue(const char *text, int64_t len, lc_queue_hist **out) {
    Parser ps{text, text + len, text};
    auto h = std::make_unique<lc_queue_hist>();
    bool unsupported = false;
    for (;;) {
        ps.ws();
        if (ps.p >= ps.end) break;
        if (*ps.p == '{') {
            if (!read_queue_op(ps, *h, unsupported)) break;
        } else if (*ps.p == '[') {  // a vector of op maps
            ++ps.p;
            bool closed = false;
            for (;;) {
                ps.ws();
                if (ps.p >= ps.end) { ps.fail("unterminated history vector"); break; }
                if (*ps.p == ']') { ++ps.p; closed = true; break; }
                if (*ps.p != '{') { ps.fail("expected an op map"); break; }
                if (!read_queue_op(ps, *h, unsupported)) break;
            }
            if (!closed) break;
        } else {
            ps.fail("expected an op map");
            break;
        }
    }
    if (!ps.err.empty())
        return lc::fail(unsupported ? LC_E_UNSUPPORTED : LC_E_PARSE, "lc_edn_queue: line %lld: %s",
                        (long long)line_of(text, ps.err_off), ps.err.c_str());
    *out = h.release();
    return LC_OK;
}

}  // namespace

extern "C" int lc_edn_parse_queue(const char *text, int64_t len, lc_queue_hist **out) {
    lc::Range range("lc_edn_parse_queue");
    if (!text || !out || len < 0) return lc::fail(LC_E_INVALID, "lc_edn_parse_queue: null argument");
    try {
        return parse_queue(text, len, out);
    } catch (const std::bad_alloc &) {
        return lc::fail(LC_E_NOMEM, "lc_edn_queue: out of memory");
    }
}

extern "C" int lc_edn_read_queue(const char *path, lc_queue_hist **out) {
    if (!path || !out) return lc::fail(LC_E_INVALID, "lc_edn_read_queue: null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return lc::fail(LC_E_IO, "lc_edn_read_queue: cannot open %s", path);
    std::string s;
    try {
        char buf[1 << 16];
        size_t r;
        while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, r);
    } catch (const std::bad_alloc &) {
        std::fclose(f);
        return lc::fail(LC_E_NOMEM, "lc_edn_read_queue: out of memory");
    }
    std::fclose(f);
    return lc_edn_parse_queue(s.data(), (int64_t)s.size(), out);
}

extern "C" int lc_queue_hist_view(const lc_queue_hist *h, lc_queue_history *out) {
    if (!h || !out) return lc::fail(LC_E_INVALID, "lc_queue_hist_view: null argument");
    out->n = (int64_t)h->type.size();
    out->type = h->type.data(); out->f = h->f.data(); out->key = h->key.data(); out->value = h->value.data();
    out->drain_off = h->drain_off.data(); out->drain_val = h->drain_val.data();
    return LC_OK;
}

extern "C" void lc_queue_hist_free(lc_queue_hist *h) { delete h; }
