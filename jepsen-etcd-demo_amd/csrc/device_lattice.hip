// device_lattice.hip -- the register tier's unsegmented search
// (k_search_lattice: one wavefront per key over a work list) and the
// validation launch (k_validate).  The lattice: lattice_core.hpp.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/lincheck.h"

#ifdef LC_T0_PROFILE
// Diagnostic build only: cycles and counts per event class (invoke, :ok with
// <= 6, 7, 8, 9, 10 pending), summed over every key.  Defined ahead of the
// include: lattice_walk's T0_PROF_* are these in this unit, whose kernel
// flushes the LDS counters, and empty in every other.
namespace lcd {
__device__ unsigned long long lc_t0_prof[12];
__shared__ unsigned long long lc_t0_prof_lds[12];
extern "C" int lc_debug_t0_prof(unsigned long long *host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lc_t0_prof), sizeof(lc_t0_prof), 0, hipMemcpyDeviceToHost);
}
}  // namespace lcd
#define T0_PROF_BEGIN const unsigned long long pt0 = __builtin_amdgcn_s_memtime(); const uint32_t pn0 = n;
#define T0_PROF_END(evi)                                                                   \
    {                                                                                      \
        const unsigned long long pt1 = __builtin_amdgcn_s_memtime();                       \
        const uint32_t cat = !((evi) & LC_EV_OK_BIT) ? 0u : (pn0 <= 6 ? 1u : pn0 - 5u);    \
        if (lane == 0 && cat < 6) { lc_t0_prof_lds[cat] += pt1 - pt0; lc_t0_prof_lds[6 + cat] += 1; } \
    }
#endif

#include "lattice_core.hpp"
#include "lattice_validate.hpp"

namespace lcd {

uint32_t t0_max_width() { return T0_MAX_WIDTH; }
uint32_t t0_max_states() { return T0_MAX_STATES; }

#ifdef LC_T0_COUNT_SWEEPS
// Diagnostic build only: the (closure width, sweeps run) histogram of every
// unit whose kernels run ok_lane -- this one and device_spec.hip (EX walks).
int spec_sweep_hist(unsigned long long *host);
extern "C" int lc_debug_sweep_hist(unsigned long long *host) {
    unsigned long long spec[8 * 8];
    int e = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lc_sweep_hist), sizeof(lc_sweep_hist), 0, hipMemcpyDeviceToHost);
    if (!e) e = spec_sweep_hist(spec);
    for (int i = 0; i < 8 * 8 && !e; ++i) host[i] += spec[i];
    return e;
}
#endif

// T0 over a work list: one wavefront per key (lattice in 4 registers, or the
// workspace for 9-10 pending ops); a persistent grid so the workspace stays
// one slot per resident block.
#ifdef LC_T0_STAMPS
// Diagnostic build only: per-block clock stamps and hardware placement.
__device__ unsigned long long lc_t0_stamps[8192 * 6];
#endif

template <bool GEN>
__global__ __launch_bounds__(64) void k_validate(T0Args a) {
    for (int64_t k = blockIdx.x; k < a.n_order; k += gridDim.x) validate_key<GEN>(a, k);
}

template <int RM>
__global__ __launch_bounds__(64) void k_search_lattice(T0Args a) {
    __shared__ uint32_t ws[3 * T0_RMEM * 64];  // lattices of 9-10 pending ops (12 KB)

#ifdef LC_T0_STAMPS
    const unsigned long long st0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
    uint32_t nkeys = 0, lastkey = 0;
#endif
#ifdef LC_T0_PROFILE
    if (lane_id() < 12) lc_t0_prof_lds[lane_id()] = 0;
#endif
    const bool fast = !(a.flags & (T0_COUNT | T0_WANT_PEAK | T0_WANT_FINAL)) && a.budget >= 16ull * 64u * 32u;
    for (int32_t guard = 0; guard <= a.n_order; ++guard) {  // every wave takes at most n_order keys
        int32_t w = 0;
        if (lane_id() == 0) w = (int32_t)((uint32_t)atomicAdd(a.ticket, 1) - a.ticket_base);
        w = __builtin_amdgcn_readfirstlane(w);
        if ((uint32_t)w >= (uint32_t)a.n_order) break;
        const int32_t key = a.order[w];
        const int kr = fast ? lattice_key<RM, true>(a, key, ws) : lattice_key<RM, false>(a, key, ws);
        if (kr == K_SPILL) t0_spill(a, key);
#ifdef LC_T0_STAMPS
        ++nkeys;
        lastkey = (uint32_t)key;
#endif
    }
#ifdef LC_T0_PROFILE
    if (lane_id() < 12) atomicAdd(&lc_t0_prof[lane_id()], lc_t0_prof_lds[lane_id()]);
#endif
#ifdef LC_T0_STAMPS
    if (lane_id() == 0 && blockIdx.x < 8192) {
        unsigned long long *o = lc_t0_stamps + blockIdx.x * 6;
        o[0] = st0; o[1] = __builtin_amdgcn_s_memtime(); o[2] = rt0; o[3] = __builtin_amdgcn_s_memrealtime();
        o[4] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4)    // HW_REG_HW_ID
               | ((unsigned long long)lastkey << 32);
        o[5] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) | ((unsigned long long)nkeys << 32);  // XCC_ID
    }
#endif
}

#ifdef LC_T0_STAMPS
extern "C" int lc_debug_t0_stamps(unsigned long long *host, int n_blocks) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(lc_t0_stamps), (size_t)n_blocks * 6 * 8, 0, hipMemcpyDeviceToHost);
}
#endif

size_t lat_ws_words() { return 3 * T0_RMEM * 64; }

// Every block ends with exactly one ticket past the work list, so a launch
// leaves the ticket at ticket_base + n_order + grid: back-to-back launches
// can start from there instead of re-zeroing it.
hipError_t launch_t0(const Args &a, const Args *a_dev, int grid, bool wide, hipStream_t s, uint32_t ticket_base) {
    T0Args t = make_t0(a, a_dev);
    t.ticket_base = ticket_base;
    if (wide) hipLaunchKernelGGL(k_search_lattice<T0_RBIG>, dim3(grid), dim3(64), 0, s, t);
    else hipLaunchKernelGGL(k_search_lattice<T0_RSMALL>, dim3(grid), dim3(64), 0, s, t);
    return hipGetLastError();
}

hipError_t launch_validate(const Args &a, hipStream_t s, bool general) {
    T0Args t{};
    t.ev_off = a.ev_off; t.events = a.events; t.trans = a.trans; t.trans_off = a.trans_off;
    t.key_states = a.key_states; t.key_error = a.key_error; t.err = a.err; t.key_width = a.key_width;
    t.err_base = a.err_base;
    t.n_order = a.n_order; t.shared_states = a.shared_states; t.n_trans = a.n_trans;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(a.n_order, 2048));
    if (general) hipLaunchKernelGGL(k_validate<true>, dim3(grid), dim3(64), 0, s, t);
    else hipLaunchKernelGGL(k_validate<false>, dim3(grid), dim3(64), 0, s, t);
    return hipGetLastError();
}

}  // namespace lcd
