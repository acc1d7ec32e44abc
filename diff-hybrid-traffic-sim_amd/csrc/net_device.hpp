// net_device.hpp -- device helpers shared by the road-network kernels (network_kernels.hip, hybrid_kernels.hip, netstep_kernels.hip, netstep_hybrid.hip, the *_step.inc).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dhts.h"
#include "arz_device.hpp"    // glue_y_bwd
#include "host_common.hpp"   // raise_fault

namespace dhts {

constexpr float kSigK = 32.f;       // sigmoid constant of the signals (_env.py:928-960, _simulator.py:128)

// The exponential of a sigmoid.  `exact` (a wave-uniform flag): the double exponential rounded once instead of the device library's expf
// (1 ulp).  The reference evaluates torch.sigmoid on CPU float32 tensors; its exp, glibc's expf and a correctly rounded exp
// agree on all but a fraction of a per cent of arguments, the device's expf differs from them on many.  One ulp in one value is
// harmless -- but in itscp `micro` mode (every lane an IDM lane stepped in float32 tensor arithmetic, a hundred vehicles following
// each other for hundreds of steps) the signals and head-gap scores steer a chaotic system, and a fuzz run over random schedules saw
// such ulps grow to 1.1-1.8e-5 of the largest queue term in 4 of 2 760 episodes (profiles/r06z_fuzz_*.log; 0 of 2 760 with the
// exact form).  The kernels ask for it exactly there: dhts_hybrid_tables::micro_tensor_ladder networks, signals and head gaps of
// differentiable episodes (+3-7 % on those episodes; every other network keeps expf and its speed).
// Two forms of it.  Out of line (kInl = false, the default): its forty instructions and their registers stay out of the callers' hot
// paths -- inlined, the persistent stepwise kernel of a network that never takes it ran 6 % slower, and the 128-register instantiation
// of the fused forward kernel 40 %.  Inline (kInl = true): what the fused kernels' roomier instantiations take -- a call costs config
// 4's forward sweep 4 %.
__device__ __forceinline__ float sig_exp_exact_inl(float x) { return (float)exp((double)x); }
__device__ __attribute__((noinline)) float sig_exp_exact_call(float x) { return (float)exp((double)x); }
template <bool kInl = false> __device__ __forceinline__ float sig_exp(float x, bool exact) {
    return exact ? (kInl ? sig_exp_exact_inl(x) : sig_exp_exact_call(x)) : expf(x);
}

// dmath/operation.py:3-30
template <bool kInl = false> __device__ __forceinline__ float soft_switch(float value, float constant, bool exact = false) {
    float z = value * constant;
    z = fminf(fmaxf(z, -16.f), 16.f);
    return 1.f / (1.f + sig_exp<kInl>(-z, exact));
}
// both at once (the reverse sweeps' loss taps): one exponential and one division instead of two of each; the same values
// (outside the clamp the gradient is 0 and the switch is the clamped one, inside z is not changed by the clamp)
template <bool kInl = false>
__device__ __forceinline__ void soft_switch_both(float value, float constant, float &s, float &ds, bool exact = false) {
    const float z = value * constant;
    const float zc = fminf(fmaxf(z, -16.f), 16.f);
    s = 1.f / (1.f + sig_exp<kInl>(-zc, exact));
    ds = (z < -16.f || z > 16.f) ? 0.f : s * (1.f - s) * constant;
}
__device__ __forceinline__ float soft_switch_grad(float value, float constant) {
    const float z = value * constant;
    if (z < -16.f || z > 16.f) return 0.f;
    const float s = 1.f / (1.f + expf(-z));
    return s * (1.f - s) * constant;
}

// ---- the ghost exchange of a road network and its adjoint (_simulator.py:42-137, road_network.py:79-111): ONE definition for the fused
// macro and hybrid kernels and the stepwise, persistent and batched ones.  float32, operation for operation what the reference's tensors
// do: the 0.f * and * 0.0f terms carry NaN and infinity.  (The tests' own restatements of this math stay apart on purpose: they judge it.)
// upstream ghost: the source lane's last cell (gr, gu) where the gate's switch s is green, an empty road (0, um) where it is red
__device__ __forceinline__ void ghost_up_blend(float gr, float gu, float s, float um, float &fr, float &fu) {
    fr = gr * s + 0.f * (1.0f - s); fu = gu * s + um * (1.0f - s);
}
// downstream ghost: the next lane's first cell (or the lane's stored ghost) where the lane's own switch s2 is green, a jam (1, 0) where red
__device__ __forceinline__ void ghost_down_blend(float gr, float gu, float s2, float &fr, float &fu) {
    fr = s2 * gr + (1.0f - s2) * 1.0f; fu = s2 * gu + (1.0f - s2) * 0.0f;
}
// Adjoints: from the step's cotangent (gg_r, gg_y) of the ghost's (r, y) to the cotangent (g_fr, g_fu) of the blended (r, u).  The caller
// multiplies it by the switch for the source cell or the stored ghost and, under its guard, takes the switch's cotangent from the one-liners.
// A downstream ghost is also the ghost the lane stores: gg_r comes summed with the stored ghost's cotangent of r, gg_u is that of u.
// (References: a caller's LDS operand is read where it is used, after the blend -- the fused reverse kernel keeps its instructions.)
__device__ __forceinline__ void ghost_up_bwd(float grn_r, float grn_u, float s, float um, const float &gg_r, const float &gg_y, float &g_fr, float &g_fu) {
    float fr, fu; ghost_up_blend(grn_r, grn_u, s, um, fr, fu);
    g_fr = gg_r; g_fu = 0.f; glue_y_bwd(fr, fu, um, gg_y, g_fr, g_fu);
}
__device__ __forceinline__ void ghost_down_bwd(float grn_r, float grn_u, float s2, float um, const float &gg_r, const float &gg_u, const float &gg_y,
                                               float &g_fr, float &g_fu) {
    float fr, fu; ghost_down_blend(grn_r, grn_u, s2, fr, fu);
    g_fr = gg_r; g_fu = gg_u; glue_y_bwd(fr, fu, um, gg_y, g_fr, g_fu);
}
__device__ __forceinline__ float ghost_up_switch_bwd(float g_fr, float g_fu, float grn_r, float grn_u, float um) { return g_fr * grn_r + g_fu * (grn_u - um); }
__device__ __forceinline__ float ghost_down_switch_bwd(float g_fr, float g_fu, float grn_r, float grn_u) { return g_fr * (grn_r - 1.0f) + g_fu * grn_u; }
// Slope of a phase signal (phase_signal_at below) w.r.t. the action entry a at progress pr, of_we: the west-east signal's, else the north-south
// one's: d sigmoid(k x) / d x = s (1 - s) k with the sigmoid values just computed, 0 outside the clamp (like the operator) and for hard signals
__device__ __forceinline__ float signal_slope(float we, float ns, float a, float pr, bool hard, bool of_we) {
    const float zs = (a - pr) * kSigK;
    const bool sat = hard || zs < -16.f || zs > 16.f;
    return sat ? 0.f : (of_we ? we * (1.f - we) * kSigK : -(ns * (1.f - ns) * kSigK));
}
__device__ __forceinline__ void signal_slopes(float we, float ns, float a, float pr, bool hard, float &dwe, float &dns) {   // both, for a table
    dwe = signal_slope(we, ns, a, pr, hard, true); dns = signal_slope(we, ns, a, pr, hard, false);
}

// Workgroup barrier that only drains LDS traffic.  __syncthreads() also waits for every outstanding global load / store
// (vmcnt(0)), which would serialise the one-step-ahead fetches of these kernels with their barriers; all data the
// phases exchange goes through LDS, and nothing a kernel writes to global memory is read back by another thread of it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Inclusive prefix sums over the 64 lanes of a wavefront with DPP moves only (no LDS crossbar round trips): row_shr 1/2/4/8
// inside the rows of 16 lanes, then row_bcast15 into rows 1 and 3 and row_bcast31 into rows 2 and 3.  Lanes without a DPP
// source add the identity.
namespace dpp {
constexpr int kRowShr1 = 0x111, kRowShr2 = 0x112, kRowShr4 = 0x114, kRowShr8 = 0x118, kBcast15 = 0x142, kBcast31 = 0x143;
template <int kCtrl, int kRowMask>
__device__ __forceinline__ int mov0(int x) { return __builtin_amdgcn_update_dpp(0, x, kCtrl, kRowMask, 0xF, false); }
template <int kCtrl, int kRowMask>
__device__ __forceinline__ double mov0(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = mov0<kCtrl, kRowMask>((int)(b & 0xffffffffll)), hi = mov0<kCtrl, kRowMask>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
}  // namespace dpp
template <typename T>
__device__ __forceinline__ T wave_scan_add(T x) {
    x += dpp::mov0<dpp::kRowShr1, 0xF>(x);
    x += dpp::mov0<dpp::kRowShr2, 0xF>(x);
    x += dpp::mov0<dpp::kRowShr4, 0xF>(x);
    x += dpp::mov0<dpp::kRowShr8, 0xF>(x);
    x += dpp::mov0<dpp::kBcast15, 0xA>(x);
    x += dpp::mov0<dpp::kBcast31, 0xC>(x);
    return x;
}
// inclusive prefix sum inside each row of 16 lanes (lane 15 of a row ends up with the row's total)
template <typename T>
__device__ __forceinline__ T row_scan_add(T x) {
    x += dpp::mov0<dpp::kRowShr1, 0xF>(x);
    x += dpp::mov0<dpp::kRowShr2, 0xF>(x);
    x += dpp::mov0<dpp::kRowShr4, 0xF>(x);
    x += dpp::mov0<dpp::kRowShr8, 0xF>(x);
    return x;
}
__device__ __forceinline__ int wave_last(int x) { return __builtin_amdgcn_readlane(x, 63); }
__device__ __forceinline__ double wave_last(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

struct NetTables {
    const int32_t *lane_ncell, *lane_off, *sig_kind, *inter;   // [L]
    const double *lane_dx;                                      // [L]
    const int32_t *left_src, *left_gate, *right_src;            // [T][L] (per replica when table_stride != 0)
    const double *schedule;                                     // [T][L]
    size_t table_stride;                                        // elements between replicas in the [T][L] tables (0 = shared)
    const int32_t *nxt_ptr, *nxt_idx, *prv_ptr, *prv_idx;       // static adjacency, CSR, ascending ids
    int n_edges;
};

// phase signals of intersection k at step t: west-east and north-south switches and their inputs (_env.py:885-962).
// `phase_raw` = t / F and `frame` = t % F are passed in so that rollouts can count them instead of dividing every step.
// hard = an evaluation episode (differentiable = False): float(a > progress), float(progress > a) (_env.py:928-960).
template <bool kInl = false>
__device__ __forceinline__ void phase_signal_at(const float *action, int n_action, int sq, int F, int phase_raw, int frame, int k,
                                                float &we, float &ns, float &a, float &prog, int &a_index, bool hard = false,
                                                bool exact = false) {
    const int last = n_action / sq - 1;
    const int phase = phase_raw > last ? last : phase_raw;
    double pr = (double)frame / (double)F;
    pr = pr > 1.0 ? 1.0 : pr;
    a_index = phase * sq + k;
    a = action[a_index];
    prog = (float)pr;
    if (hard) { we = a > prog ? 1.f : 0.f; ns = prog > a ? 1.f : 0.f; return; }
    we = soft_switch<kInl>(a - prog, kSigK, exact);
    ns = soft_switch<kInl>(prog - a, kSigK, exact);
}
__device__ __forceinline__ void phase_signal(const float *action, int n_action, int sq, int F, int t, int k,
                                             float &we, float &ns, float &a, float &prog, int &a_index) {
    phase_signal_at(action, n_action, sq, F, t / F, t % F, k, we, ns, a, prog, a_index);
}

}  // namespace dhts
