// host_common.hpp -- what the host halves of the translation units share: the code between a C ABI entry point and a kernel launch,
// the option variables dhts_set_option (dhts_common.hip) writes, and the one fault record helper every kernel uses.
// A family's launch decisions live in its plan (MacroPlan, MicroPlan, HybPlan, NsPlan): computed once, read by the launch AND by the
// family's dhts_*_plan entry point.  Nothing here enters the device code but raise_fault, which is inlined into its callers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/dhts.h"

namespace dhts {

// the first fault of a launch wins: its thread fills the record
__device__ __forceinline__ void raise_fault(dhts_error *err, int code, int step, int lane, int index) {
    if (err == nullptr) return;
    if (atomicCAS(&err->code, 0, code) == 0) {
        err->step = step;
        err->lane = lane;
        err->index = index;
    }
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? DHTS_OK : DHTS_E_LAUNCH; }
// workgroups of 256 threads for n items of a grid-stride kernel
inline int grid_1d(int64_t n, int cap = 2048) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
constexpr int padded64(int n) { return (n + 63) & ~63; }

// Let `kernel` take `lds` bytes of dynamic LDS.  The runtime is asked at every launch that needs it (no record of what was set).
inline bool set_max_lds(const void *kernel, size_t lds) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}
// ... where it exceeds what a kernel may take unasked.  The persistent and stepwise network kernels ask from 48 KB on (kNsLdsDefault,
// netstep_hybrid.hip), every other family from 64 KB on.  What a failure returns is the entry point's own business (DHTS_E_LAUNCH
// or DHTS_E_INVALID: part of the ABI).
constexpr size_t kLdsDefault = 64 * 1024;
template <class K>
inline bool allow_lds(K kernel, size_t lds, size_t unasked = kLdsDefault) {
    return lds <= unasked || set_max_lds((const void *)kernel, lds);
}
// the one spelling of a launch: a family writes its argument list once and passes the instantiation
template <class K, class... A>
inline void launch(K kernel, dim3 grid, dim3 block, size_t lds, void *stream, const A &...args) {
    kernel<<<grid, block, lds, (hipStream_t)stream>>>(args...);
}

// both: false when the limit could not be raised (nothing was launched then)
template <class K, class... A>
inline bool launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, size_t unasked, void *stream, const A &...args) {
    if (!allow_lds(kernel, lds, unasked)) return false;
    launch(kernel, grid, block, lds, stream, args...);
    return true;
}

// Run-time value -> template argument: calls f(std::integral_constant<int, V>{}) for the V of the list that equals v (false: none
// does).  A family's plan names the instantiation in ints; the launch picks it with this and writes its argument list once.
// A list is also the set of instantiations the library holds: name what a plan can name and nothing else; a combination a kernel
// rules out is left out with `if constexpr` in f.  Editing a list changes the library's device-code fingerprint (bench.py
// library_code_sha16, profiles/issue_counters.json) even where no kernel changes, so the counter record is re-taken afterwards.
template <int... Vs, class F>
inline bool pick(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// The tangent sweeps (dhts_macro_rollout_jvp, dhts_micro_rollout_jvp) run n directions as launches of 4, then 2, then 1: the width of
// the instantiation that carries the next launch, `rem` directions left, at most `kmax` (4, 2 or 1) per launch.  A remainder of 3
// rides in ONE launch of 4 with a slot masked (the tape is read once instead of twice).
inline int jvp_width(int rem, int kmax) {
    if (rem >= 3 && kmax >= 4) return 4;
    int k = kmax < 2 ? kmax : 2;
    while (k > rem) k >>= 1;
    return k;
}
// n_dir directions as those launches: f(k0, integral_constant<kK>, n_act) per launch -- first direction, the instantiation's slots,
// the directions it carries -- until one returns false (-> false).  kmax = 0 (no launch fits the lane): f is not called.
template <class F>
inline bool jvp_each_group(int n_dir, int kmax, F &&f) {
    bool ok = true;
    for (int k0 = 0; k0 < n_dir && kmax > 0 && ok;) {
        const int kk = jvp_width(n_dir - k0, kmax), n_act = kk < n_dir - k0 ? kk : n_dir - k0;
        pick<4, 2, 1>(kk, [&](auto kv) { ok = f(k0, kv, n_act); });
        k0 += n_act;
    }
    return ok;
}
// ... and what a plan says of them: the slots of the widest (the first) launch, the number of launches
struct JvpGroups { int widest, launches; };
inline JvpGroups jvp_groups(int kmax, int n_dir) {
    JvpGroups g = {0, 0};
    jvp_each_group(n_dir, kmax, [&](int, auto kv, int) {
        if (!g.launches) g.widest = decltype(kv)::value;
        ++g.launches;
        return true;
    });
    return g;
}

}  // namespace dhts

// ---- option variables: each lives in its family's file; dhts_set_option (dhts_common.hip) holds the accepted values ----
extern int dhts_fwd_waves_override;          // macro_kernels.hip, DHTS_OPT_MACRO_FWD_WAVES
extern int dhts_fwd_variant;                 // macro_kernels.hip, DHTS_OPT_MACRO_FWD_VARIANT
extern int dhts_fwd_rotate;                  // macro_kernels.hip, DHTS_OPT_MACRO_FWD_ROTATE
extern int dhts_fwd_group;                   // macro_kernels.hip, DHTS_OPT_MACRO_FWD_GROUP
extern int dhts_jvp_variant;                 // macro_kernels.hip, DHTS_OPT_MACRO_JVP_VARIANT
extern int dhts_micro_fwd_waves_override;    // micro_kernels.hip, DHTS_OPT_MICRO_FWD_WAVES
extern int dhts_netstep_block;               // netstep_hybrid.hip, DHTS_OPT_NETSTEP_BLOCK
extern int dhts_netstep_lds_kb;              // netstep_hybrid.hip, DHTS_OPT_NETSTEP_LDS_KB
extern int dhts_hyb_pack;                    // hybrid_kernels.hip, DHTS_OPT_HYB_PACK
extern int dhts_opt_reward_chain;            // dhts_common.hip, DHTS_OPT_REWARD_CHAIN

// dhts_common.hip: the reward as the reference's one float32 chain, lanes outermost (what DHTS_OPT_REWARD_CHAIN turns on)
int dhts_launch_reward_chain(int R, int T, int L, const float *queue, const int32_t *lane_macro, int hard, double dt, int loss_steps,
                             float *reward, int stride, void *stream);
