// micro_kernels.hip -- time-fused forward and reverse sweeps of the IDM car-following ODE on gfx950.
//
// Forward (micro_rollout_fwd_kernel<K>): one 64-lane wavefront owns one traffic lane for the whole rollout.
//   Vehicle slot i follows slot i + 1 (MicroLane.curr_vehicle order), so the leader of a vehicle is simply the
//   next slot: positions and speeds (float32) live in LDS, thread t of pass j owns slot 64 j + t, its six
//   double parameters stay in registers for all T steps (K = passes is a template parameter so they do), and
//   passes run tail -> head so that a pass reads its leaders' OLD state before the next pass overwrites it.
//   HBM sees the initial load, the final store and the Jacobian tape (32 B per vehicle-step, two coalesced
//   16-B-per-lane streams).  The head vehicle uses the lane's (head_position_delta, head_speed_delta).
// Reverse (micro_rollout_bwd_kernel): one workgroup per lane, cotangent in LDS, newest step first:
//   g'[i] = dEgo[i]^T g[i] + dLeading[i-1]^T g[i-1]; the virtual-leader slot's cotangent returns to the head
//   vehicle and to the head gap (dmicro_lane.py:130-153, 271-298).
// Tangent (micro_rollout_jvp_kernel, micro_jvp.inc): the same blocks untransposed, oldest step first, K directions per pass over the tape.
// Fused (micro_rollout_fwd_jvp_kernel, micro_fwd_jvp.inc): the forward and K tangent directions stepped together, no tape at all.
// Checkpointed (micro_rollout_ckpt_fwd_kernel / _bwd_kernel, micro_ckpt.inc): reverse mode with the state kept every S steps and the tape
//   of one segment at a time rebuilt in LDS.
// Sampled (micro_rollout_ckpt_fwd_samples_kernel / _bwd_samples_kernel, micro_rollout_fwd_jvp_samples_kernel): the two tape-free paths
//   writing and reading probe samples [T / every][L][2][P] in place of a [T][L][2][V] history -- the same two files, included again.
// Recorded leader (the kLead = true instantiations of the three sampled kernels): the head vehicle follows lead [T][L][2], a vehicle
//   given per step, instead of a constant head gap; its cotangent per step is g_lead, its tangents t_lead.
// Ring road (the kBoundRing instantiations of the same kernels and of the two target kernels): the head follows the lane's own tail
//   one circumference ahead; the image's cotangent returns to the tail, its tangents are the tail's.
//
// Reference: road/lane/_micro_lane.py:131-214, road/lane/dmicro_lane.py:87-127 and :271-298.
#include <hip/hip_runtime.h>

#include "../../include/dhts.h"
#include "arz_device.hpp"   // dot2
#include "host_common.hpp"
#include "idm_device.hpp"

namespace dhts {

// compact rollout tape entry: (dEgo[1][0], dEgo[1][1], dLeading[1][1]).  The first rows of both blocks are constants
// ([1, dt] and [0, 0]) and dLeading[1][0] = -dEgo[1][0] bit for bit: dt * (2 a s^2 / gap^3) against dt * (-2 a s^2 / gap^3),
// both 0 under the acceleration clip (didm.py:38-103) -- 12 bytes per vehicle-step instead of the 32 of dqs[V][2][2][2]
struct __attribute__((packed, aligned(4))) MicroTape3 { float e2, e3, l3; };

// The parameter tape (dhts_micro_param_tape_bytes; opaque to callers): a 64-byte header that names the shape it was written for, the
// lanes' head gaps [L][2] double (the reverse sweep is not handed them) rounded up to whole 64 bytes, then [step][lane][Vp] float2 =
// the (p, v) a vehicle entered the step with: 8 B per vehicle-step.
struct ParamTapeHeader { int32_t magic, L, V, T; int32_t pad[12]; };
constexpr int32_t kParamTapeMagic = 0x50544431;
__host__ __device__ inline ParamTapeHeader param_tape_header(int L, int V, int T) {
    ParamTapeHeader h = {};
    h.magic = kParamTapeMagic; h.L = L; h.V = V; h.T = T;
    return h;
}
__host__ __device__ inline size_t param_tape_steps_offset(int L) { return sizeof(ParamTapeHeader) + (((size_t)L * 16 + 63) & ~(size_t)63); }

// grid = L workgroups of 64 * kW threads; dynamic LDS = 2 * (V + 1) floats (kW = 1) or twice that (kW > 1: the state
// ping-pongs between two buffers so that one workgroup barrier per step separates a step's reads from the next step's).
// kW wavefronts per lane: thread `tid` of pass j owns slot (64 kW) j + tid.
// kFull: every slot of every lane holds a vehicle (no counts, V = 64 kW K): no validity masks, no index clamps, and only the
// last pass can hold the head vehicle.
// kParams: the rollout will be differentiated with respect to the driver parameters too: beside the tape, every step writes the
// operands of its IDM evaluation that the reverse sweep cannot rebuild -- the vehicle's pre-step (p, v) -- into the parameter tape
// (layout: ParamTapeHeader below).  Same arithmetic, same tape, same outputs as without it.
template <int K, int kW, bool kCompact, bool kFull, bool kParams = false>
__global__ __launch_bounds__(64 * kW) void micro_rollout_fwd_kernel(
    int L, int V, int T, double dt,
    const float *__restrict__ p_in, const float *__restrict__ v_in, const int32_t *__restrict__ count,
    const double *__restrict__ params, const double *__restrict__ head,
    float *__restrict__ p_out, float *__restrict__ v_out, float *__restrict__ tape, float *__restrict__ hist,
    dhts_error *err, char *__restrict__ ptape = nullptr) {
    extern __shared__ float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    constexpr int kStride = 64 * kW;
    float *Sp = lds, *Sv = lds + (V + 1);
    const size_t base = (size_t)lane * V;
    const int n = (!kFull && count) ? count[lane] : V;
    const int Vp = (V + 63) & ~63;
    const size_t plane = (size_t)L * V;

    IdmDerived prm[K];
    double len_lead[K];
    const double inv_dt = 1.0 / dt;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = j * kStride + t;
        const int ic = i < V ? i : V - 1;
        const int il = (i + 1) < V ? (i + 1) : V - 1;
        IdmParams raw;
        raw.a_max = params[0 * plane + base + ic];
        raw.a_pref = params[1 * plane + base + ic];
        raw.v_target = params[2 * plane + base + ic];
        raw.min_space = params[3 * plane + base + ic];
        raw.time_pref = params[4 * plane + base + ic];
        raw.length = params[5 * plane + base + ic];
        prm[j] = idm_derive(raw);
        idm_set_dt(prm[j], dt);
        len_lead[j] = params[5 * plane + base + il];
    }
    for (int k = t; k < V; k += kStride) { Sp[k] = p_in[base + k]; Sv[k] = v_in[base + k]; }
    if (t == 0) { Sp[V] = 0.f; Sv[V] = 0.f; if (kW > 1) { Sp[2 * (V + 1) + V] = 0.f; Sv[2 * (V + 1) + V] = 0.f; } }
    __syncthreads();
    const double head_dp = head[(size_t)lane * 2], head_dv = head[(size_t)lane * 2 + 1];
    int fault_step = -1, fault_index = 0;
    float2 *pt0 = nullptr;
    if constexpr (kParams) {
        if (t == 0) {
            if (lane == 0) *reinterpret_cast<ParamTapeHeader *>(ptape) = param_tape_header(L, V, T);
            double *ph = reinterpret_cast<double *>(ptape + sizeof(ParamTapeHeader)) + (size_t)lane * 2;
            ph[0] = head_dp; ph[1] = head_dv;
        }
        pt0 = reinterpret_cast<float2 *>(ptape + param_tape_steps_offset(L)) + (size_t)lane * Vp;
    }

    for (int step = 0; step < T; ++step) {
        float4 *tp = (tape && !kCompact) ? reinterpret_cast<float4 *>(tape) + ((size_t)step * L + lane) * 2 * Vp : nullptr;
        MicroTape3 *tc = (tape && kCompact) ? reinterpret_cast<MicroTape3 *>(tape) + ((size_t)step * L + lane) * Vp : nullptr;
        float *hp = hist ? hist + ((size_t)step * L + lane) * 2 * V : nullptr;
        // every pass reads its own and its leaders' OLD state before anything is written, so the K IDM evaluations of a
        // thread are independent instruction streams (a wave's LDS operations execute in order: no barrier is needed
        // between this step's writes and the next step's reads)
        // kW > 1: read buffer (step & 1), write the other one
        const float *Rp = Sp + ((kW > 1 && (step & 1)) ? 2 * (V + 1) : 0), *Rv = Sv + ((kW > 1 && (step & 1)) ? 2 * (V + 1) : 0);
        float *Wp = Sp + ((kW > 1 && !(step & 1)) ? 2 * (V + 1) : 0), *Wv = Sv + ((kW > 1 && !(step & 1)) ? 2 * (V + 1) : 0);
        float rp[K], rv[K], rpl[K], rvl[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = j * kStride + t;
            const int ic = (kFull || i < n) ? i : 0;
            rp[j] = Rp[ic]; rv[j] = Rv[ic]; rpl[j] = Rp[ic + 1]; rvl[j] = Rv[ic + 1];
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = j * kStride + t;
            const bool valid = kFull || i < n;
            const double p = rp[j], v = rv[j];
            const double pl = rpl[j], vl = rvl[j];
            double dp, dv;
            if ((!kFull || j == K - 1) && i == n - 1) {      // compute_state_delta, _micro_lane.py:201-204
                dp = head_dp; dv = head_dv;
            } else {                                  // :206-212
                dp = fabs(pl - p) - ((len_lead[j] + prm[j].length) * 0.5);
                dv = v - vl;
            }
            IdmStep o;
            idm_step(p, v, dp, dv, prm[j], dt, inv_dt, o);
            if (valid) {
                if (o.collided && fault_step < 0) { fault_step = step; fault_index = i; }
                Wp[i] = o.np; Wv[i] = o.nv;
                if constexpr (kCompact) {
                    if (tc) { MicroTape3 e; e.e2 = o.dE[2]; e.e3 = o.dE[3]; e.l3 = o.dLd[3]; tc[i] = e; }
                } else if (tp) {
                    tp[i] = make_float4(o.dE[0], o.dE[1], o.dE[2], o.dE[3]);
                    tp[Vp + i] = make_float4(o.dLd[0], o.dLd[1], o.dLd[2], o.dLd[3]);
                }
                if (hp) { hp[i] = o.np; hp[V + i] = o.nv; }
                if constexpr (kParams) pt0[(size_t)step * L * Vp + i] = make_float2(rp[j], rv[j]);
            }
        }
        if constexpr (kW > 1) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // LDS-only: tape stores stay in flight
    }
    __syncthreads();
    const float *Fp = Sp + ((kW > 1 && (T & 1)) ? 2 * (V + 1) : 0), *Fv = Sv + ((kW > 1 && (T & 1)) ? 2 * (V + 1) : 0);
    // slots >= count pass through: a step writes only live slots, and with kW > 1 and an odd T the final buffer is the one the
    // initial load never filled
    for (int k = t; k < V; k += kStride) { p_out[base + k] = k < n ? Fp[k] : p_in[base + k]; v_out[base + k] = k < n ? Fv[k] : v_in[base + k]; }
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_COLLISION, fault_step, lane, fault_index);
}

// known-answer entry: n independent vehicles.  in [9][n] double = a_max a_pref v v_target dp dv min_space time_pref dt
__global__ void idm_batch_kernel(int64_t n, int variant, const double *__restrict__ in, double *__restrict__ next_pv,
                                 float *__restrict__ dE, float *__restrict__ dLd, int32_t *__restrict__ collided,
                                 double *__restrict__ acc_s, int32_t *__restrict__ clips) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        IdmParams m;
        m.a_max = in[i]; m.a_pref = in[n + i]; m.v_target = in[3 * n + i]; m.min_space = in[6 * n + i];
        m.time_pref = in[7 * n + i]; m.length = 0.;
        IdmStep o;
        const double dt = in[8 * n + i];
        if (variant == 1) idm_step_ieee(0.0, in[2 * n + i], in[4 * n + i], in[5 * n + i], m, dt, o);
        else { IdmDerived dm = idm_derive(m); idm_set_dt(dm, dt); idm_step(0.0, in[2 * n + i], in[4 * n + i], in[5 * n + i], dm, dt, 1.0 / dt, o); }
        next_pv[i] = o.np; next_pv[n + i] = o.nv;
        collided[i] = o.collided ? 1 : 0;
        acc_s[i] = o.acc; acc_s[n + i] = o.sstar;
        clips[i] = o.clipped_acc ? 1 : 0; clips[n + i] = o.clipped_spacing ? 1 : 0;
        for (int j = 0; j < 4; ++j) { dE[j * n + i] = o.dE[j]; dLd[j * n + i] = o.dLd[j]; }
    }
}

// known-answer entry of the Jacobians ALONE, with the caller's optimal spacing and clip flags (dIDM.compute_dEgo / compute_dLeading
// take them as arguments, didm.py:13-103: the reference's lane passes flags derived from the CLAMPED gap beside the un-clamped gap
// itself, dmicro_lane.py:97).  in [12][n] double = a_max a_pref v v_target dp dv min_space time_pref optimal_spacing dt
// clipped_acceleration clipped_optimal_spacing
__global__ void idm_jac_batch_kernel(int64_t n, const double *__restrict__ in, float *__restrict__ dE, float *__restrict__ dLd) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double a_max = in[i], a_pref = in[n + i], v = in[2 * n + i], v_t = in[3 * n + i], dp = in[4 * n + i], dv = in[5 * n + i];
        const double time_pref = in[7 * n + i], s = in[8 * n + i], dt = in[9 * n + i];
        const bool clipped_a = in[10 * n + i] != 0., clipped_s = in[11 * n + i] != 0.;
        float e[4] = {1.f, (float)dt, 0.f, 0.f}, l[4] = {0.f, 0.f, 0.f, 0.f};
        if (!clipped_a) {
            const double dp2 = dp * dp, dp3 = dp2 * dp;
            const double s2_dp3 = (s * s) / dp3, s_dp2 = s / dp2;
            const double vt2 = v_t * v_t;
            const double free_term = -4.0 * ((v * v * v) / (vt2 * vt2));
            const double two_sqrt_ab = 2 * sqrt(a_max * a_pref);
            e[2] = (float)(dt * (-2 * a_max * s2_dp3));
            l[2] = (float)(dt * (2 * a_max * s2_dp3));
            if (clipped_s) {
                e[3] = (float)(1 + dt * a_max * free_term);
                l[3] = (float)(dt * a_max * (-2 * s_dp2));
            } else {
                e[3] = (float)(1 + dt * a_max * (free_term - 2 * s_dp2 * (time_pref + ((v + dv) / two_sqrt_ab))));
                l[3] = (float)(dt * a_max * (-2 * s_dp2 * (-v / two_sqrt_ab)));
            }
        }
        for (int j = 0; j < 4; ++j) { dE[j * n + i] = e[j]; dLd[j * n + i] = l[j]; }
    }
}

// known-answer entry of the parameter partials ALONE (idm_param_jac, the function the reverse sweep calls): n independent operand
// sets, in [9][n] double as idm_batch_kernel's with the RAW gap; the collision rule and the clamp are the lane's (a gap the forward
// replaced by a constant has no partial).  dacc [6][n] = d acc / d (a_max, a_pref, v_target, min_space, time_pref, gap)
__global__ void idm_param_jac_batch_kernel(int64_t n, const double *__restrict__ in, double *__restrict__ dacc, int32_t *__restrict__ clips) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        IdmParams m;
        m.a_max = in[i]; m.a_pref = in[n + i]; m.v_target = in[3 * n + i]; m.min_space = in[6 * n + i];
        m.time_pref = in[7 * n + i]; m.length = 0.;
        const double v = in[2 * n + i], dt = in[8 * n + i];
        double gap = in[4 * n + i], dv = in[5 * n + i];
        const bool live_gap = gap >= 1e-5;
        if (gap < 0) { gap = 0; dv = 0; }
        gap = (1e-5 > gap) ? 1e-5 : gap;
        IdmParamJac pj;
        idm_param_jac(v, gap, dv, idm_param_derive(m), dt, pj);
        for (int q = 0; q < 6; ++q) dacc[q * n + i] = (pj.clipped_acc || (q == 5 && !live_gap)) ? 0. : pj.d[q];
        clips[i] = pj.clipped_acc ? 1 : 0; clips[n + i] = pj.clipped_spacing ? 1 : 0;
    }
}

// grid = L workgroups of blockDim.x threads; dynamic LDS = 4 * (V + 2) floats (kParams: 6 * (V + 2))
// kParams: the sweep also sums, per vehicle, gv dt d acc / d theta over the steps (gv = the cotangent of the vehicle's speed AFTER the
// step, g_hist term included): the partials are recomputed in double from the parameter tape's pre-step (p, v), the leader's (through
// LDS) and the vehicle's parameters in registers; the acceleration clip is the forward's own decision, read off the tape entry (all
// three zero).  Six double sums per thread, added in step order -- no atomics.  One vehicle per thread only: the launch sizes the
// block to the lane (up to 1024 threads), a smaller block is reported as DHTS_FAULT_CAPACITY and g_params is NaN.
// The state recurrence is the same instructions on the same values: g_p_out, g_v_out, g_head are those of the sweep without it.
template <bool kCompact, bool kParams = false>
__global__ void micro_rollout_bwd_kernel(
    int L, int V, int T, double dt, const float *__restrict__ tape, const int32_t *__restrict__ count,
    const float *__restrict__ g_p_in, const float *__restrict__ g_v_in, const float *__restrict__ g_hist,
    float *__restrict__ g_p_out, float *__restrict__ g_v_out, double *__restrict__ g_head, int fold, dhts_error *err,
    const char *__restrict__ ptape = nullptr, const double *__restrict__ params = nullptr, double *__restrict__ g_params = nullptr) {
    extern __shared__ float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    const int B = blockDim.x;
    const int P = V + 2;
    float *Gp = lds, *Gv = lds + P, *C1p = lds + 2 * P, *C1v = lds + 3 * P;   // C1[i + 1] = dLeading[i]^T g[i]
    const size_t base = (size_t)lane * V;
    const int n = count ? count[lane] : V;
    const int Vp = (V + 63) & ~63;

    for (int k = t; k < P; k += B) { Gp[k] = 0.f; Gv[k] = 0.f; C1p[k] = 0.f; C1v[k] = 0.f; }
    __syncthreads();
    for (int k = t; k < n; k += B) { Gp[k] = g_p_in[base + k]; Gv[k] = g_v_in[base + k]; }
    __syncthreads();

    double gh_p = 0., gh_v = 0.;       // held by the thread that owns the head vehicle
    int bad_step = -1, bad_index = 0;  // first non-finite cotangent this thread meets (the latest step: the sweep runs backwards)
    int step_hi = T - 1;
    // kParams: this thread's vehicle, its sums, and whether the parameter tape is the one a forward of this shape wrote
    float *Xp = lds + 4 * P, *Xv = lds + 5 * P;        // pre-step state of the step being replayed (kParams only)
    IdmParamDerived pm = {};
    double half_len = 0., head_dp = 0., head_dv = 0.;
    double sum[6] = {0., 0., 0., 0., 0., 0.};           // a_max, a_pref, v_target, min_space, time_pref, gap
    bool pt_ok = false;
    if constexpr (kParams) {
        const ParamTapeHeader h = *reinterpret_cast<const ParamTapeHeader *>(ptape);
        pt_ok = h.magic == kParamTapeMagic && h.L == L && h.V == V && h.T == T && V <= B;
        if (pt_ok && t < n) {
            const size_t plane = (size_t)L * V;
            IdmParams raw;
            raw.a_max = params[0 * plane + base + t]; raw.a_pref = params[1 * plane + base + t];
            raw.v_target = params[2 * plane + base + t]; raw.min_space = params[3 * plane + base + t];
            raw.time_pref = params[4 * plane + base + t]; raw.length = params[5 * plane + base + t];
            pm = idm_param_derive(raw);
            half_len = (params[5 * plane + base + (t + 1 < n ? t + 1 : t)] + raw.length) * 0.5;
            const double *ph = reinterpret_cast<const double *>(ptape + sizeof(ParamTapeHeader)) + (size_t)lane * 2;
            head_dp = ph[0]; head_dv = ph[1];
        }
    }
    if constexpr (kCompact) {
        if (V <= B && T > 0) {         // (T = 0: no tape to prefetch from -- the tape pointer may be NULL)
            // One vehicle per thread (the rollouts' common shape): the tape entry of the NEXT step to replay is loaded while
            // this step computes (unconditional load, clamped step index), and the barriers wait for LDS only, so the load
            // stays in flight across them -- the tape stream is what bounds this kernel.  Per-step cotangents (a loss on the
            // state history) travel the same way.
            const int k = t;
            const bool vk = k < n;
            const MicroTape3 *tc0 = reinterpret_cast<const MicroTape3 *>(tape) + (size_t)lane * Vp + (k < V ? k : 0);
            const size_t step_stride = (size_t)L * Vp;
            MicroTape3 nx = tc0[(size_t)(T - 1) * step_stride];
            MicroTape3 nx2 = tc0[(size_t)(T > 1 ? T - 2 : 0) * step_stride];
            const float *gh0 = g_hist ? g_hist + (size_t)lane * 2 * V + (k < V ? k : 0) : nullptr;
            const size_t h_stride = (size_t)L * 2 * V;
            float hp1 = 0.f, hv1 = 0.f, hp2 = 0.f, hv2 = 0.f;
            if (gh0) {
                const float *a = gh0 + (size_t)(T - 1) * h_stride, *b = gh0 + (size_t)(T > 1 ? T - 2 : 0) * h_stride;
                hp1 = a[0]; hv1 = a[V]; hp2 = b[0]; hv2 = b[V];
            }
            const float dtf = (float)dt;
            // (a tape of another shape is never read: the loads stay on its header)
            const float2 *pt0 = reinterpret_cast<const float2 *>(ptape + ((kParams && pt_ok) ? param_tape_steps_offset(L) : 0)) +
                                ((kParams && pt_ok) ? (size_t)lane * Vp + (k < V ? k : 0) : 0);
            const size_t pstride = (kParams && pt_ok) ? step_stride : 0;
            float2 px = make_float2(0.f, 0.f), px2 = px;
            if constexpr (kParams) { px = pt0[(size_t)(T - 1) * pstride]; px2 = pt0[(size_t)(T > 1 ? T - 2 : 0) * pstride]; }
            for (int step = T - 1; step >= 0; --step) {
                const MicroTape3 c = nx;
                const float chp = hp1, chv = hv1;
                nx = nx2; hp1 = hp2; hv1 = hv2;
                nx2 = tc0[(size_t)(step > 1 ? step - 2 : 0) * step_stride];       // two steps ahead
                const float2 cx = px;
                float gv_step = 0.f;
                if constexpr (kParams) { px = px2; px2 = pt0[(size_t)(step > 1 ? step - 2 : 0) * pstride]; }
                if (gh0) { const float *a = gh0 + (size_t)(step > 1 ? step - 2 : 0) * h_stride; hp2 = a[0]; hv2 = a[V]; }
                if (vk) {
                    float gp = Gp[k], gv = Gv[k];
                    if (gh0) { gp += chp; gv += chv; }
                    Gp[k] = dot2(1.f, gp, c.e2, gv);           // grad_ps[:-1] = dqs[:, 0]^T g
                    Gv[k] = dot2(dtf, gp, c.e3, gv);
                    C1p[k + 1] = dot2(0.f, gp, -c.e2, gv);     // grad_ps[1:] += dqs[:, 1]^T g
                    C1v[k + 1] = dot2(0.f, gp, c.l3, gv);
                    if constexpr (kParams) { Xp[k] = cx.x; Xv[k] = cx.y; gv_step = gv; }
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if constexpr (kParams) {
                    if (vk && pt_ok) {
                        // compute_state_delta and the collision / clamp rules of the forward, _micro_lane.py:149-166, 201-212
                        const bool is_head = k == n - 1;
                        const double pv = cx.y;
                        double gap = is_head ? head_dp : fabs((double)Xp[k + 1] - (double)cx.x) - half_len;
                        double dv = is_head ? head_dv : pv - (double)Xv[k + 1];
                        const bool live_gap = !is_head && gap >= 1e-5;       // else a constant: nothing flows to the lengths
                        if (gap < 0) { gap = 0; dv = 0; }
                        gap = (1e-5 > gap) ? 1e-5 : gap;
                        if (!(c.e2 == 0.f && c.e3 == 0.f && c.l3 == 0.f)) {  // (the forward's acceleration clip zeroes all three)
                            IdmParamJac pj;
                            idm_param_jac(pv, gap, dv, pm, dt, pj);
                            const double w = (double)gv_step * dt;
#pragma unroll
                            for (int q = 0; q < 5; ++q) sum[q] += w * pj.d[q];
                            if (live_gap) sum[5] += w * pj.d[5];
                        }
                    }
                }
                if (vk) {
                    float np_ = Gp[k], nv_ = Gv[k];
                    if (k > 0) { np_ += C1p[k]; nv_ += C1v[k]; }
                    if (k == n - 1) {
                        const float vp = C1p[n], vv = C1v[n];
                        if (fold) {
                            gh_p += (double)vp;
                            gh_v -= (double)vv;
                            np_ += vp; nv_ += vv;
                        } else {
                            gh_p = (double)vp;
                            gh_v = (double)vv;
                        }
                    }
                    Gp[k] = np_; Gv[k] = nv_;
                    // a gap clamped to 0 makes the IDM Jacobian divide by it (didm.py:60-70) and the sweep meet 0 * inf.  The
                    // reference's micro backward hands such NaNs on silently (dmicro_lane.py:271-298 has no assert, unlike
                    // dmacro_lane.py:308); the values are kept, and the fault record says where the first one appeared
                    if (bad_step < 0 && !(isfinite(np_) && isfinite(nv_))) { bad_step = step; bad_index = k; }
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            step_hi = -1;
            __syncthreads();
        }
    }
    for (int step = step_hi; step >= 0; --step) {
        const float4 *tp = reinterpret_cast<const float4 *>(tape) + ((size_t)step * L + lane) * 2 * Vp;            // reference layout
        const MicroTape3 *tc = reinterpret_cast<const MicroTape3 *>(tape) + ((size_t)step * L + lane) * Vp;         // compact layout
        const float *gh = g_hist ? g_hist + ((size_t)step * L + lane) * 2 * V : nullptr;
        for (int k = t; k < n; k += B) {
            float4 dE, dLd;
            if constexpr (kCompact) {
                const MicroTape3 c = tc[k];
                dE = make_float4(1.f, (float)dt, c.e2, c.e3); dLd = make_float4(0.f, 0.f, -c.e2, c.l3);
            } else { dE = tp[k]; dLd = tp[Vp + k]; }
            float gp = Gp[k], gv = Gv[k];
            if (gh) { gp += gh[k]; gv += gh[V + k]; }
            Gp[k] = dot2(dE.x, gp, dE.z, gv);          // grad_ps[:-1] = dqs[:, 0]^T g
            Gv[k] = dot2(dE.y, gp, dE.w, gv);
            C1p[k + 1] = dot2(dLd.x, gp, dLd.z, gv);   // grad_ps[1:] += dqs[:, 1]^T g
            C1v[k + 1] = dot2(dLd.y, gp, dLd.w, gv);
        }
        __syncthreads();
        for (int k = t; k < n; k += B) {
            float np_ = Gp[k], nv_ = Gv[k];
            if (k > 0) { np_ += C1p[k]; nv_ += C1v[k]; }
            if (k == n - 1) {
                // virtual leader = (p_head + head_dp, v_head - head_dv): its cotangent C1[n] returns to the head
                const float vp = C1p[n], vv = C1v[n];
                if (fold) {
                    gh_p += (double)vp;
                    gh_v -= (double)vv;
                    np_ += vp; nv_ += vv;
                } else {                   // single-step operator form: hand the raw slot cotangent back
                    gh_p = (double)vp;
                    gh_v = (double)vv;
                }
            }
            Gp[k] = np_; Gv[k] = nv_;
            if (bad_step < 0 && !(isfinite(np_) && isfinite(nv_))) { bad_step = step; bad_index = k; }
        }
        __syncthreads();
    }
    for (int k = t; k < V; k += B) {
        g_p_out[base + k] = (k < n) ? Gp[k] : 0.f;
        g_v_out[base + k] = (k < n) ? Gv[k] : 0.f;
    }
    if constexpr (kParams) {
        // length enters a gap as -(len_leader + len) / 2 (_micro_lane.py:211): a vehicle's own gap sum and its follower's
        double *A = reinterpret_cast<double *>(C1p);            // (C1p, C1v: 2 P floats = P doubles; the sweeps are done with them)
        __syncthreads();
        if (t < V) A[t] = (t < n) ? sum[5] : 0.;
        __syncthreads();
        if (t < V) {
            const size_t plane = (size_t)L * V;
            const bool live = t < n;
            const double nan = __builtin_nan("");
#pragma unroll
            for (int q = 0; q < 5; ++q) g_params[q * plane + base + t] = !pt_ok ? nan : (live ? sum[q] : 0.);
            g_params[5 * plane + base + t] = !pt_ok ? nan : (live ? -0.5 * (A[t] + (t > 0 ? A[t - 1] : 0.)) : 0.);
        }
        if (!pt_ok && t == 0) raise_fault(err, DHTS_FAULT_CAPACITY, 0, lane, -3);      // not this shape's parameter tape (or block < lane)
    }
    if (g_head) {
        if (n == 0) { if (t == 0) { g_head[(size_t)lane * 2] = 0.; g_head[(size_t)lane * 2 + 1] = 0.; } }
        else if (t == (n - 1) % B) { g_head[(size_t)lane * 2] = gh_p; g_head[(size_t)lane * 2 + 1] = gh_v; }
    }
    // the lane's report: the latest step at which a non-finite cotangent appeared (the first the sweep met), lowest vehicle
    __shared__ int s_bad;
    if (t == 0) s_bad = -1;
    __syncthreads();
    if (bad_step >= 0) atomicMax(&s_bad, (bad_step << 10) | (1023 - bad_index));      // capacity <= 1024 vehicles
    __syncthreads();
    if (t == 0 && s_bad >= 0) raise_fault(err, DHTS_FAULT_NAN, s_bad >> 10, lane, 1023 - (s_bad & 1023));
}

// The single-step operator in the float32 TENSOR ladder (idm_step_f32): what the reference's plain MicroLane computes when its vehicle
// states are torch tensors -- itscp `micro` mode, differentiable episodes (example/control/itscp/_env.py:484-498; _micro_lane.py:131-214
// evaluated by torch).  One thread per vehicle slot; same tape as dhts_micro_step_fwd ([lane][2][Vp][4]), same reverse operator.
// kHeadOnly: the head vehicle alone meets a float32 tensor (its gap) -- mixed arithmetic for it, double for the followers (idm_step_lane)
template <bool kHeadOnly>
__global__ void micro_step_tensor_fwd_kernel(int L, int V, double dt, const float *__restrict__ p_in, const float *__restrict__ v_in,
                                             const int32_t *__restrict__ count, const double *__restrict__ params,
                                             const double *__restrict__ head, float *__restrict__ p_out, float *__restrict__ v_out,
                                             float *__restrict__ tape, dhts_error *err) {
    const int lane = blockIdx.x;
    const size_t base = (size_t)lane * V, plane = (size_t)L * V;
    const int n = count ? count[lane] : V;
    const int Vp = (V + 63) & ~63;
    float4 *tp = tape ? reinterpret_cast<float4 *>(tape) + (size_t)lane * 2 * Vp : nullptr;
    int fault_index = -1;
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
        if (i >= n) { p_out[base + i] = p_in[base + i]; v_out[base + i] = v_in[base + i]; continue; }
        IdmParams m;
        m.a_max = params[0 * plane + base + i]; m.a_pref = params[1 * plane + base + i]; m.v_target = params[2 * plane + base + i];
        m.min_space = params[3 * plane + base + i]; m.time_pref = params[4 * plane + base + i]; m.length = params[5 * plane + base + i];
        const float pi = p_in[base + i], vi = v_in[base + i];
        float dp, dv;
        if (i == n - 1) { dp = (float)head[(size_t)lane * 2]; dv = (float)head[(size_t)lane * 2 + 1]; }
        else {
            const double len_l = params[5 * plane + base + i + 1];
            dp = fabsf(p_in[base + i + 1] - pi) - (float)((len_l + m.length) * 0.5);
            dv = vi - v_in[base + i + 1];
        }
        IdmStep o;
        if constexpr (kHeadOnly) {
            double dpd, dvd;
            if (i == n - 1) { dpd = (double)(float)head[(size_t)lane * 2]; dvd = (double)(float)head[(size_t)lane * 2 + 1]; }
            else {
                const double len_l = params[5 * plane + base + i + 1];
                dpd = fabs((double)p_in[base + i + 1] - (double)pi) - ((len_l + m.length) * 0.5);
                dvd = (double)vi - (double)v_in[base + i + 1];
            }
            idm_step_lane(pi, vi, dpd, dvd, i == n - 1, m, dt, o);
        } else {
            const float sg = i == n - 1 ? 1.f : (p_in[base + i + 1] > pi ? 1.f : (p_in[base + i + 1] < pi ? -1.f : 0.f));
            idm_step_f32(pi, vi, dp, dv, m, dt, o, sg);
        }
        if (o.collided && fault_index < 0) fault_index = i;
        p_out[base + i] = o.np; v_out[base + i] = o.nv;
        if (tp) {
            tp[i] = make_float4(o.dE[0], o.dE[1], o.dE[2], o.dE[3]);
            tp[Vp + i] = make_float4(o.dLd[0], o.dLd[1], o.dLd[2], o.dLd[3]);
        }
    }
    if (fault_index >= 0) raise_fault(err, DHTS_FAULT_COLLISION, 0, lane, fault_index);
}

// ---- forward-mode tangent sweep over the rollout tape (dhts_micro_rollout_jvp) ----------------------------------
#include "micro_jvp.inc"
// ---- probe samples of the two tape-free paths (dhts_micro_rollout_*_samples) --------------------------------------
// Which slots are observed and how often: row j of a samples array [T / every][L][2][n] holds (p, v) -- or their tangents, or their
// cotangents -- of slot probes[i] in column i after step (j + 1) every - 1; the trailing T mod every steps have no row.
struct MicroProbes {
    const int32_t *probes;   // [n] distinct slots, or NULL: every slot, column i = slot i (n = V)
    int n;                   // columns of a row
    int every;               // >= 1
};
// The column slot k has among the probes, -1 for none: read once by the thread that owns the slot, before its step loop.  An entry
// outside [0, V) equals no slot, so no address is ever formed from one and its column stays as the caller left it.
__device__ inline int micro_probe_column(const MicroProbes &pr, int k, int V) {
    if (k >= V) return -1;
    if (pr.probes == nullptr) return k;
    int col = -1;
    for (int i = 0; i < pr.n; ++i) col = pr.probes[i] == k ? i : col;
    return col;
}
// a block smaller than the lane (DHTS_FAULT_CAPACITY): the lane's part of every row of one samples array takes `value`
__device__ inline void micro_samples_fill(float *samples, const MicroProbes &pr, int T, int L, int lane, int k, int B, float value) {
    const int rows = T / pr.every;
    for (int j = 0; j < rows; ++j)
        for (int i = k; i < 2 * pr.n; i += B) samples[((size_t)j * L + lane) * 2 * pr.n + i] = value;
}
// ---- a recorded leader on the two tape-free paths (dhts_micro_rollout_*_lead) -------------------------------------
// kLead forms of the three sampled kernels: the lane's head vehicle (slot count - 1) follows a prescribed vehicle whose state `in`
// step t is row t of lead, as every other vehicle follows the slot in front of it; no virtual leader and no head gap exist.
struct MicroLead {
    const float *lead;       // [T][L][2] (p, v) the head sees in step t
    const double *length;    // [L] the leader's length, or NULL: the head's own
    float *g_lead;           // reverse sweep: [T][L][2], every row written
    const float *t_lead;     // fused JVP: [kK][T][L][2] of this launch's directions, or NULL: zero
    const double *ring;      // kBoundRing: [L] the circumference of each lane's ring; the four above are then unused
};
// What the head vehicle (slot count - 1) follows, a template parameter of the three sampled and the two target kernels: the constant
// head gap, the recorded leader above, or -- the ring road, dhts_micro_rollout_*_ring -- the image of the lane's own tail (slot 0) one
// circumference ahead: slot n of S holds ((float)((double)p_tail + ring[lane]), v_tail), written by the TAIL's thread beside its own
// store, and the head is an ordinary follower of it (include/dhts.h).  Positions stay unwrapped.
enum MicroBoundary { kBoundHead = 0, kBoundLead = 1, kBoundRing = 2 };
// This lane's entry of row 0 of a [T][L][2] array, for the ONE thread that walks the rows (the head vehicle's).  The address is the
// same for a whole workgroup, so without the opaque zero the rows would be read by scalar loads, which the step's LDS-only wait
// (lgkmcnt) also waits for; from a vector register they are vector loads and stay in flight across it, as g_hist rows do.
__device__ inline const float *micro_lead_row(const float *rows, int lane) {
    int z = 0;
    asm volatile("" : "+v"(z));
    return rows + (size_t)lane * 2 + z;
}
// the lane's entry of every row of g_lead takes `value` (a lane without a vehicle: 0; a block smaller than the lane: NaN)
__device__ inline void micro_lead_fill(float *g_lead, int T, int L, int lane, int k, int B, float value) {
    for (int t = k; t < T; t += B) { g_lead[((size_t)t * L + lane) * 2] = value; g_lead[((size_t)t * L + lane) * 2 + 1] = value; }
}
// ---- the rollout and its tangents in one kernel, no tape (dhts_micro_rollout_fwd_jvp) ----------------------------
#define DHTS_MICRO_SAMPLES 0
#include "micro_fwd_jvp.inc"
// ---- reverse mode from checkpoints, the segment tape in LDS (dhts_micro_rollout_fwd_ckpt / _bwd_ckpt) -------------
#include "micro_ckpt.inc"
// ---- the sampled forms of the three kernels of the two files (dhts_micro_rollout_*_samples): the same text again ----
#undef DHTS_MICRO_SAMPLES
#define DHTS_MICRO_SAMPLES 1
#include "micro_fwd_jvp.inc"
#include "micro_ckpt.inc"
#undef DHTS_MICRO_SAMPLES
// ---- the trajectory-fit loss inside the checkpointed pair (dhts_micro_rollout_*_ckpt_target): the text of micro_ckpt.inc once more ----
#define DHTS_MICRO_SAMPLES 2
#include "micro_ckpt.inc"
#undef DHTS_MICRO_SAMPLES
// ---- the Gauss-Newton normal equations inside the fused kernel (dhts_micro_rollout_fwd_jvp_gn): the text of micro_fwd_jvp.inc once more ----
#define DHTS_MICRO_SAMPLES 3
#include "micro_fwd_jvp.inc"
#undef DHTS_MICRO_SAMPLES

}  // namespace dhts

using namespace dhts;

static inline bool micro_desc_ok(const dhts_micro_desc *d) {
    return d && d->n_lanes > 0 && d->capacity > 0 && d->capacity <= DHTS_MICRO_MAX_VEHICLES && d->dt > 0;
}
int dhts_micro_fwd_waves_override = 0;      // DHTS_OPT_MICRO_FWD_WAVES: 0 = heuristic, 1 / 2 / 4 wavefronts per lane

// Which instantiations the rollout launches for a shape: read by the launches below and by dhts_micro_rollout_plan.
struct MicroPlan {
    int W, K;                // forward: wavefronts per lane (1, 2 or 4) and the literal passes per thread (1, 2, 4, 8 or 16)
    bool full;               // forward: every slot of every lane holds a vehicle (kFull)
    int bwd_block;           // reverse: threads per lane
    bool bwd_per_thread;     // reverse: the one-vehicle-per-thread sweep (the kernel's own test: the lane fits the block and there is a tape)
    // the rollout that is differentiated w.r.t. the driver parameters too (dhts_micro_rollout_fwd_params / _bwd_params)
    int ptape_bytes;         // parameter tape, bytes per vehicle-step: 8 = the pre-step (p, v), partials recomputed in the reverse sweep
    int pbwd_block;          // its reverse sweep: threads per lane -- the whole lane, one vehicle per thread holds its six double sums
    // the tangent sweep (dhts_micro_rollout_jvp, micro_jvp.inc)
    int jvp_block;           // threads per lane: the whole lane, one vehicle per thread holds its tangents
    int jvp_kmax;            // directions a launch may carry: 4, with t_params too (6 double tangents each: 128 VGPRs, no scratch)
    // the tape-free fused forward + tangent kernel (dhts_micro_rollout_fwd_jvp, micro_fwd_jvp.inc)
    int fwd_jvp_block;       // threads per lane: the whole lane, one vehicle per thread holds its state and its tangents
    int fwd_jvp_kmax[2];     // directions a launch may carry, [0] state-only, [1] with t_params
    // the checkpointed pair (dhts_micro_rollout_fwd_ckpt / _bwd_ckpt, micro_ckpt.inc)
    int ckpt_block;          // threads per lane of both kernels: the whole lane, one vehicle per thread
    struct Ring {
        int max_segment[2];  // steps the reverse kernel's ring can hold within kCkptLdsBudget, [0] state-only, [1] with g_params
        int segment;         // the segment length a caller gets who names none (one value for both reverse kernels: the forward
                             // that writes the checkpoints does not know which of them will read them)
    } ckpt[2];               // [0] the hist and sampled forms, [1] the target forms (dhts_micro_rollout_*_ckpt_target): the same
                             // block and rule, a ring with the two target planes
};
constexpr size_t kCkptLdsBudget = 160 * 1024;      // LDS of a CU: what one workgroup may take
// The default segment: the longest, up to kCkptSegmentCap, whose reverse workgroup (sized with the parameter ring) still leaves
// kCkptWavesPerCu wavefronts resident on a CU by LDS -- a longer segment divides the checkpoint bytes further, but the sweep is a
// chain of LDS-only barriers that only other resident workgroups hide (DESIGN.md section 4e has the sweep both were set from).
constexpr int kCkptSegmentCap = 16;
constexpr int kCkptWavesPerCu = 16;
static MicroPlan micro_plan(const dhts_micro_desc *d, int T, bool has_count) {
    MicroPlan pl;
    // wavefronts per lane: one wave keeps the whole lane free of barriers; with few lanes per SIMD more waves per lane buy
    // the latency hiding back (256 CUs x 4 SIMDs x 8 waves)
    int W = dhts_micro_fwd_waves_override;
    if (W == 0) W = (d->capacity > 64 && (long long)d->n_lanes * 2 <= 8192) ? 2 : 1;
    pl.W = (W >= 4 && d->capacity > 128) ? 4 : ((W >= 2 && d->capacity > 64) ? 2 : 1);
    const int K = (d->capacity + 64 * pl.W - 1) / (64 * pl.W);
    pl.K = K <= 1 ? 1 : (K <= 2 ? 2 : (K <= 4 ? 4 : (K <= 8 ? 8 : 16)));
    pl.full = !has_count && d->capacity == 64 * pl.W * pl.K;
    pl.bwd_block = padded64(d->capacity) > 256 ? 256 : padded64(d->capacity);
    pl.bwd_per_thread = d->capacity <= pl.bwd_block && T > 0;
    pl.ptape_bytes = (int)sizeof(float2);
    pl.pbwd_block = padded64(d->capacity);
    pl.jvp_block = padded64(d->capacity);
    pl.jvp_kmax = 4;
    pl.fwd_jvp_block = padded64(d->capacity);
    pl.fwd_jvp_kmax[0] = 4;
    pl.fwd_jvp_kmax[1] = 4;
    pl.ckpt_block = padded64(d->capacity);
    const int waves = pl.ckpt_block / 64;
    const int groups = (kCkptWavesPerCu + waves - 1) / waves;                    // workgroups per CU that make kCkptWavesPerCu
    const size_t fixed = micro_ckpt_bwd_fixed_bytes(d->capacity);
    const long long room = (long long)(kCkptLdsBudget / groups) - (long long)fixed;
    for (int target = 0; target < 2; ++target) {
        MicroPlan::Ring &ring = pl.ckpt[target];
        for (int q = 0; q < 2; ++q)
            ring.max_segment[q] = (int)((kCkptLdsBudget - fixed) / micro_ckpt_bwd_step_bytes(d->capacity, q != 0, target != 0));
        int S = room > 0 ? (int)(room / (long long)micro_ckpt_bwd_step_bytes(d->capacity, true, target != 0)) : 0;
        S = S > kCkptSegmentCap ? kCkptSegmentCap : S;
        S = S > ring.max_segment[1] ? ring.max_segment[1] : S;
        ring.segment = S < 1 ? 1 : S;
    }
    return pl;
}
// the segment a call runs with: the caller's, or the plan's for 0; -1 where the reverse kernel's ring cannot hold it
static int micro_ckpt_segment(const MicroPlan::Ring &ring, int segment, bool params) {
    if (segment < 0 || segment > ring.max_segment[params ? 1 : 0]) return -1;
    return segment == 0 ? ring.segment : segment;
}
static int micro_ckpt_count(int T, int S) { return T > 0 ? (T + S - 1) / S : 0; }
// the 8 ints of dhts_micro_ckpt_plan (target false) and dhts_micro_ckpt_target_plan (true)
static int micro_ckpt_plan_fill(const dhts_micro_desc *d, int T, bool params, int segment, bool target, int32_t plan[8]) {
    if (!micro_desc_ok(d) || T < 0 || !plan) return DHTS_E_INVALID;
    const MicroPlan pl = micro_plan(d, T, false);
    const int S = micro_ckpt_segment(pl.ckpt[target], segment, params);
    if (S < 0) return DHTS_E_INVALID;
    const size_t bwd_lds = micro_ckpt_bwd_lds_bytes(d->capacity, S, params, target);
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = pl.ckpt_block;
    plan[1] = S;
    plan[2] = pl.ckpt[target].max_segment[params ? 1 : 0];
    plan[3] = micro_ckpt_count(T, S);
    plan[4] = (int32_t)micro_ckpt_fwd_lds_bytes(d->capacity);
    plan[5] = (int32_t)bwd_lds;
    plan[6] = (int32_t)(kCkptLdsBudget / bwd_lds);
    return DHTS_OK;
}

template <bool kCompact, bool kParams = false>
static int micro_fwd_launch(const dhts_micro_desc *d, int T,
                            const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                            float *p_out, float *v_out, float *tape, float *hist, dhts_error *err, void *stream, char *ptape = nullptr) {
    if (!micro_desc_ok(d) || T < 0 || !p || !v || !params || !head || !p_out || !v_out) return DHTS_E_INVALID;
    if (kParams && (!ptape || (T > 0 && !tape))) return DHTS_E_INVALID;      // (the reverse sweep reads the acceleration clip off the tape)
    const MicroPlan pl = micro_plan(d, T, count != nullptr);
    const size_t lds = sizeof(float) * (pl.W > 1 ? 4 : 2) * (size_t)(d->capacity + 1);
    pick<1, 2, 4>(pl.W, [&](auto w) {
        pick<16, 8, 4, 2, 1>(pl.K, [&](auto k) {
            pick<0, 1>(pl.full, [&](auto full) {
                launch(micro_rollout_fwd_kernel<decltype(k)::value, decltype(w)::value, kCompact, decltype(full)::value != 0, kParams>, d->n_lanes,
                       64 * pl.W, lds, stream, d->n_lanes, d->capacity, T, d->dt, p, v, count, params, head, p_out, v_out, tape, hist, err, ptape);
            });
        });
    });
    return launch_status();
}
template <bool kCompact>
static int micro_bwd_launch(const dhts_micro_desc *d, int T, const float *tape, const int32_t *count,
                            const float *g_p, const float *g_v, const float *g_hist,
                            float *g_p_out, float *g_v_out, double *g_head, int fold, dhts_error *err, void *stream) {
    if (!micro_desc_ok(d) || T < 0 || (T > 0 && !tape) || !g_p || !g_v || !g_p_out || !g_v_out) return DHTS_E_INVALID;
    const size_t lds = sizeof(float) * 4 * (size_t)(d->capacity + 2);
    launch(micro_rollout_bwd_kernel<kCompact>, d->n_lanes, micro_plan(d, T, count != nullptr).bwd_block, lds, stream,
           d->n_lanes, d->capacity, T, d->dt, tape, count, g_p, g_v, g_hist, g_p_out, g_v_out, g_head, fold, err,
           (const char *)nullptr, (const double *)nullptr, (double *)nullptr);
    return launch_status();
}
static int micro_bwd_params_launch(const dhts_micro_desc *d, int T, const float *tape, const char *ptape, const int32_t *count,
                                   const double *params, const float *g_p, const float *g_v, const float *g_hist,
                                   float *g_p_out, float *g_v_out, double *g_head, double *g_params, dhts_error *err, void *stream) {
    if (!micro_desc_ok(d) || T < 0 || (T > 0 && !tape) || !ptape || !params || !g_params || !g_p || !g_v || !g_p_out || !g_v_out)
        return DHTS_E_INVALID;
    const size_t lds = sizeof(float) * 6 * (size_t)(d->capacity + 2);
    launch(micro_rollout_bwd_kernel<true, true>, d->n_lanes, micro_plan(d, T, count != nullptr).pbwd_block, lds, stream,
           d->n_lanes, d->capacity, T, d->dt, tape, count, g_p, g_v, g_hist, g_p_out, g_v_out, g_head, 1, err, ptape, params, g_params);
    return launch_status();
}
static int micro_jvp_launch(const dhts_micro_desc *d, int T, int n_dir, const float *tape, const char *ptape, const int32_t *count,
                            const double *params, const float *t_p, const float *t_v, const double *t_head, const double *t_params,
                            float *t_p_out, float *t_v_out, float *t_hist, dhts_error *err, void *stream) {
    const MicroPlan pl = micro_plan(d, T, count != nullptr);
    const int L = d->n_lanes, V = d->capacity;
    const size_t dir_state = (size_t)L * V, dir_hist = (size_t)T * L * 2 * V;
    const bool lds_ok = jvp_each_group(n_dir, pl.jvp_kmax, [&](int k0, auto kv, int n_act) {
        constexpr int kK = decltype(kv)::value;
        const double *a_h = t_head ? t_head + (size_t)k0 * L * 2 : nullptr, *a_q = t_params ? t_params + k0 * 6 * dir_state : nullptr;
        float *o_h = t_hist ? t_hist + k0 * dir_hist : nullptr;
        bool ok = true;
        pick<0, 1>(t_params != nullptr, [&](auto pv) {
            constexpr bool kParams = decltype(pv)::value != 0;
            ok = launch_lds(micro_rollout_jvp_kernel<kK, kParams>, L, pl.jvp_block, micro_jvp_lds_bytes(V, kK, kParams), kLdsDefault,
                            stream, L, V, T, d->dt, tape, ptape, count, params, t_p + k0 * dir_state, t_v + k0 * dir_state, a_h, a_q,
                            n_act, t_p_out + k0 * dir_state, t_v_out + k0 * dir_state, o_h, err);
        });
        return ok;
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

// The instantiations of the tape-free kernels, named once in the order the code object has held them since each form was added.  The
// launches below name them again by form; without this list their order in the code object would follow the launches, and bench.py's
// fingerprint of the device code (profiles/issue_counters.json) is over its bytes.  A new instantiation goes at the end.
[[maybe_unused]] static const void *const kMicroTapeFreeKernels[] = {
    (const void *)micro_rollout_fwd_jvp_kernel<1, true>,
    (const void *)micro_rollout_fwd_jvp_kernel<1, false>,
    (const void *)micro_rollout_fwd_jvp_kernel<2, true>,
    (const void *)micro_rollout_fwd_jvp_kernel<2, false>,
    (const void *)micro_rollout_fwd_jvp_kernel<4, true>,
    (const void *)micro_rollout_fwd_jvp_kernel<4, false>,
    (const void *)micro_rollout_ckpt_bwd_kernel<true>,
    (const void *)micro_rollout_ckpt_bwd_kernel<false>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<1, true, kBoundLead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<1, true, kBoundHead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<1, false, kBoundLead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<1, false, kBoundHead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<2, true, kBoundLead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<2, true, kBoundHead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<2, false, kBoundLead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<2, false, kBoundHead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<4, true, kBoundLead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<4, true, kBoundHead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<4, false, kBoundLead>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<4, false, kBoundHead>,
    (const void *)micro_rollout_ckpt_fwd_samples_kernel<kBoundLead>,
    (const void *)micro_rollout_ckpt_fwd_samples_kernel<kBoundHead>,
    (const void *)micro_rollout_ckpt_bwd_samples_kernel<true, kBoundLead>,
    (const void *)micro_rollout_ckpt_bwd_samples_kernel<true, kBoundHead>,
    (const void *)micro_rollout_ckpt_bwd_samples_kernel<false, kBoundLead>,
    (const void *)micro_rollout_ckpt_bwd_samples_kernel<false, kBoundHead>,
    (const void *)micro_rollout_ckpt_fwd_target_kernel<kBoundLead>,
    (const void *)micro_rollout_ckpt_fwd_target_kernel<kBoundHead>,
    (const void *)micro_rollout_ckpt_bwd_target_kernel<true, kBoundLead>,
    (const void *)micro_rollout_ckpt_bwd_target_kernel<true, kBoundHead>,
    (const void *)micro_rollout_ckpt_bwd_target_kernel<false, kBoundLead>,
    (const void *)micro_rollout_ckpt_bwd_target_kernel<false, kBoundHead>,
    (const void *)micro_rollout_ckpt_fwd_samples_kernel<kBoundRing>,
    (const void *)micro_rollout_ckpt_fwd_target_kernel<kBoundRing>,
    (const void *)micro_rollout_ckpt_bwd_samples_kernel<true, kBoundRing>,
    (const void *)micro_rollout_ckpt_bwd_samples_kernel<false, kBoundRing>,
    (const void *)micro_rollout_ckpt_bwd_target_kernel<true, kBoundRing>,
    (const void *)micro_rollout_ckpt_bwd_target_kernel<false, kBoundRing>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<1, true, kBoundRing>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<1, false, kBoundRing>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<2, true, kBoundRing>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<2, false, kBoundRing>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<4, true, kBoundRing>,
    (const void *)micro_rollout_fwd_jvp_samples_kernel<4, false, kBoundRing>};
// ---- the Gauss-Newton form of the fused kernel: which instantiations exist, what a launch carries, which launches a call takes -------
// The block bound a launch of kK directions is compiled for.  Four directions with the parameter term need 169 .. 186 VGPRs (16 double
// accumulators beside 24 parameter tangents), which a block of 1024 does not leave: that instantiation exists for 512 threads only and
// carries lanes of up to 512 slots.  Every other one fits the 128 VGPRs of 1024 threads and exists for that bound alone (a smaller
// bound compiles to the same registers).
constexpr int micro_gn_bound(int kK, bool params) { return kK >= 4 && params ? 512 : 1024; }
// The widest micro_rollout_fwd_jvp_gn_kernel a lane of V slots can be handed: every instantiation held shows no scratch and no spill
// for all three boundaries (profiles/micro_gn_resources.txt); a wider one is not instantiated, the plan narrows the launch instead.
constexpr int micro_gn_kmax(int V, bool params) { return params && V > micro_gn_bound(4, true) ? 2 : 4; }
// K directions under launch width w.  K <= w: one launch.  Otherwise the directions are cut into blocks of w / 2 and every PAIR of
// blocks gets a launch (cross products need both directions in one launch): f(first, n_act, dir) per launch, until one returns false.
// w < 2 carries K = 1 only.  Returns the number of launches, 0 where the width cannot carry K, -1 where f stopped.
template <class F>
inline int micro_gn_each_launch(int K, int w, F &&f) {
    int dir[4] = {0, 0, 0, 0};
    if (K < 1 || w < 1 || (K > w && w < 2)) return 0;
    if (K <= w) {
        for (int d = 0; d < K; ++d) dir[d] = d;
        return f(true, K, dir) ? 1 : -1;
    }
    const int h = w / 2, nb = (K + h - 1) / h;
    int launches = 0;
    for (int i = 0; i < nb; ++i)
        for (int j = i + 1; j < nb; ++j) {
            int n = 0;
            for (int d = i * h; d < (i + 1) * h && d < K; ++d) dir[n++] = d;
            for (int d = j * h; d < (j + 1) * h && d < K; ++d) dir[n++] = d;
            if (!f(launches == 0, n, dir)) return -1;
            ++launches;
        }
    return launches;
}
// ---- the tape-free paths: the fused forward + tangent kernel and the checkpointed pair, every form through three launches ----------
// The form a call runs in, host only (unpacked into the kernels' parameter lists at the launch): what it observes -- the dense
// history, probe samples or the fit to a target -- with the arrays of that kind, and the recorded leader where the head follows one.
enum MicroObserve { kObserveHist, kObserveSamples, kObserveTarget };
struct MicroForm {
    MicroObserve kind;
    MicroProbes pr;          // kObserveSamples: which slots, how often
    float *obs;              // forward: hist or samples
    float *t_obs;            // fused forward + tangent: t_hist or t_samples
    const float *g_obs;      // reverse: g_hist or g_samples
    const float *target;     // kObserveTarget, both directions
    double *sse;             // ... forward
    const double *g_sse;     // ... reverse
    const MicroLead *lead;   // the recorded leader, or (with its `ring` set) the ring road; NULL: the constant head gap
};
// which of the three the form's head vehicle follows
static int micro_form_boundary(const MicroForm &f) { return !f.lead ? kBoundHead : (f.lead->ring ? kBoundRing : kBoundLead); }
static MicroForm micro_form_hist(float *hist, float *t_hist, const float *g_hist) {
    MicroForm f = {};
    f.kind = kObserveHist; f.obs = hist; f.t_obs = t_hist; f.g_obs = g_hist;
    return f;
}
static MicroForm micro_form_samples(const MicroProbes &pr, float *samples, float *t_samples, const float *g_samples, const MicroLead *lead) {
    MicroForm f = {};
    f.kind = kObserveSamples; f.pr = pr; f.obs = samples; f.t_obs = t_samples; f.g_obs = g_samples; f.lead = lead;
    return f;
}
static MicroForm micro_form_target(const float *target, double *sse, const double *g_sse, const MicroLead *lead) {
    MicroForm f = {};
    f.kind = kObserveTarget; f.target = target; f.sse = sse; f.g_sse = g_sse; f.lead = lead;
    return f;
}
// the checks the sampled entry points share -> the kernels' MicroProbes (n = V without a list); false: DHTS_E_INVALID
static bool micro_probes_ok(const dhts_micro_desc *d, const int32_t *probes, int n_probes, int every, MicroProbes *pr) {
    if (every < 1 || (probes && (n_probes < 1 || n_probes > d->capacity))) return false;
    *pr = MicroProbes{probes, probes ? n_probes : d->capacity, every};
    return true;
}
// ... and the ones every forward and every reverse entry point of the two paths has
static bool micro_fwd_args_ok(const dhts_micro_desc *d, int T, const float *p, const float *v, const double *params, const float *p_out,
                              const float *v_out) {
    return micro_desc_ok(d) && T >= 0 && p && v && params && p_out && v_out;
}
static bool micro_bwd_args_ok(const dhts_micro_desc *d, int T, const double *params, const float *g_p, const float *g_v,
                              const float *g_p_out, const float *g_v_out) {
    return micro_desc_ok(d) && T >= 0 && params && g_p && g_v && g_p_out && g_v_out;
}
static bool micro_tangent_args_ok(int n_dir, const float *t_p, const float *t_v, const float *t_p_out, const float *t_v_out) {
    return n_dir >= 1 && t_p && t_v && t_p_out && t_v_out;
}
// The fused kernel under its own cap on the directions of a launch; every launch recomputes the primal (same bits), the first one
// alone is handed hist / samples and the forward's fault record, each its own directions of t_head, t_params, t_lead and
// t_hist / t_samples.
static int micro_fwd_jvp_launch(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                const double *params, const double *head, const float *t_p, const float *t_v, const double *t_head,
                                const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out, const MicroForm &f,
                                dhts_error *err, dhts_error *err_jvp, void *stream) {
    const MicroPlan pl = micro_plan(d, T, count != nullptr);
    const int L = d->n_lanes, V = d->capacity;
    const bool samp = f.kind == kObserveSamples;
    const size_t dir_state = (size_t)L * V, dir_lead = (size_t)T * L * 2;
    const size_t dir_obs = samp ? (size_t)(T / f.pr.every) * L * 2 * f.pr.n : (size_t)T * L * 2 * V;
    const bool lds_ok = jvp_each_group(n_dir, pl.fwd_jvp_kmax[t_params ? 1 : 0], [&](int k0, auto kv, int n_act) {
        constexpr int kK = decltype(kv)::value;
        const double *a_h = t_head ? t_head + (size_t)k0 * L * 2 : nullptr, *a_q = t_params ? t_params + k0 * 6 * dir_state : nullptr;
        float *obs = k0 == 0 ? f.obs : nullptr, *t_obs = f.t_obs ? f.t_obs + k0 * dir_obs : nullptr;
        dhts_error *err_fwd = k0 == 0 ? err : nullptr;
        MicroLead ld = f.lead ? *f.lead : MicroLead{};
        if (ld.t_lead) ld.t_lead += k0 * dir_lead;       // this launch's directions
        bool ok = true;
        pick<0, 1>(t_params != nullptr, [&](auto pv) {
            constexpr bool kParams = decltype(pv)::value != 0;
            auto go = [&](auto kernel, const auto &...observed) {
                ok = launch_lds(kernel, L, pl.fwd_jvp_block, micro_fwd_jvp_lds_bytes(V, kK), kLdsDefault, stream, L, V, T, d->dt, p, v, count,
                                params, head, t_p + k0 * dir_state, t_v + k0 * dir_state, a_h, a_q, n_act, p_out, v_out,
                                t_p_out + k0 * dir_state, t_v_out + k0 * dir_state, observed...);
            };
            if (!samp) go(micro_rollout_fwd_jvp_kernel<kK, kParams>, obs, t_obs, err_fwd, err_jvp);
            else pick<0, 1, 2>(micro_form_boundary(f), [&](auto bv) {
                go(micro_rollout_fwd_jvp_samples_kernel<kK, kParams, (MicroBoundary) decltype(bv)::value>, f.pr, obs, t_obs, err_fwd, err_jvp, ld);
            });
        });
        return ok;
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}
// The Gauss-Newton form: the launches of micro_gn_each_launch, each handed the CALL's per-direction arrays and its own direction map; the
// first alone writes p_out, v_out, sse and the forward's fault record.  An entry of jtj or jtr that several launches write receives
// the same bits from each (the same sum in the same order), so nothing is assembled afterwards and nothing races on one stream.
static int micro_fwd_jvp_gn_launch(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                   const double *params, const double *head, const float *t_p, const float *t_v, const double *t_head,
                                   const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                   const MicroProbes &pr, const MicroLead *lead, const float *target, double *sse, double *jtr, double *jtj,
                                   dhts_error *err, dhts_error *err_jvp, void *stream) {
    const int L = d->n_lanes, V = d->capacity;
    const int width = micro_gn_kmax(V, t_params != nullptr);
    const int boundary = !lead ? kBoundHead : (lead->ring ? kBoundRing : kBoundLead);
    const MicroLead ld = lead ? *lead : MicroLead{};
    const int launches = micro_gn_each_launch(n_dir, width, [&](bool first, int n_act, const int *dir) {
        MicroGn gn = {target, first ? sse : nullptr, jtr, jtj, n_dir, {dir[0], dir[1], dir[2], dir[3]}};
        bool ok = false;
        pick<4, 2, 1>(n_act >= 3 ? 4 : n_act, [&](auto kv) {
            pick<0, 1>(t_params != nullptr, [&](auto pv) {
                pick<0, 1, 2>(boundary, [&](auto bv) {
                    constexpr int kK = decltype(kv)::value;
                    constexpr bool kParams = decltype(pv)::value != 0;
                    if (padded64(V) <= micro_gn_bound(kK, kParams))      // (the plan's width never asks otherwise)
                        ok = launch_lds(micro_rollout_fwd_jvp_gn_kernel<kK, kParams, (MicroBoundary) decltype(bv)::value, micro_gn_bound(kK, kParams)>,
                                        L, padded64(V), micro_fwd_jvp_lds_bytes(V, kK), kLdsDefault, stream, L, V, T, d->dt, p, v, count,
                                        params, head, t_p, t_v, t_head, t_params, n_act, first ? p_out : nullptr,
                                        first ? v_out : nullptr, t_p_out, t_v_out, pr, gn, first ? err : nullptr, err_jvp, ld);
                });
            });
        });
        return ok;
    });
    if (launches == 0) return DHTS_E_INVALID;
    return launches > 0 ? launch_status() : DHTS_E_LAUNCH;
}
// The checkpointed pair: both read block and segment (the form's ring) off the plan; the reverse kernel asks for its LDS above 64 KB.
static int micro_ckpt_fwd_launch(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                 const double *params, const double *head, float *p_out, float *v_out, void *ckpt, const MicroForm &f,
                                 dhts_error *err, void *stream) {
    const MicroPlan pl = micro_plan(d, T, count != nullptr);
    // (a forward is valid for every segment some reverse kernel of its form can take)
    const int S = micro_ckpt_segment(pl.ckpt[f.kind == kObserveTarget], segment, false);
    if (S < 0) return DHTS_E_INVALID;
    const int L = d->n_lanes, V = d->capacity;
    const MicroLead ld = f.lead ? *f.lead : MicroLead{};
    bool ok = true;
    auto go = [&](auto kernel, const auto &...observed) {
        ok = launch_lds(kernel, L, pl.ckpt_block, micro_ckpt_fwd_lds_bytes(V), kLdsDefault, stream, L, V, T, S, d->dt, p, v, count, params,
                        head, p_out, v_out, (float2 *)ckpt, observed...);
    };
    if (f.kind == kObserveHist) go(micro_rollout_ckpt_fwd_kernel, f.obs, err);
    else pick<0, 1, 2>(micro_form_boundary(f), [&](auto bv) {
        constexpr MicroBoundary kB = (MicroBoundary) decltype(bv)::value;
        if (f.kind == kObserveSamples) go(micro_rollout_ckpt_fwd_samples_kernel<kB>, f.pr, f.obs, err, ld);
        else go(micro_rollout_ckpt_fwd_target_kernel<kB>, f.target, f.sse, err, ld);
    });
    return ok ? launch_status() : DHTS_E_LAUNCH;
}
static int micro_ckpt_bwd_launch(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count, const double *params,
                                 const double *head, const float *g_p, const float *g_v, float *g_p_out, float *g_v_out, double *g_head,
                                 double *g_params, const MicroForm &f, dhts_error *err, void *stream) {
    const MicroPlan pl = micro_plan(d, T, count != nullptr);
    const bool target = f.kind == kObserveTarget;
    const int S = micro_ckpt_segment(pl.ckpt[target], segment, g_params != nullptr);
    if (S < 0) return DHTS_E_INVALID;
    const int L = d->n_lanes, V = d->capacity;
    const float2 *ck = (const float2 *)ckpt;
    const MicroLead ld = f.lead ? *f.lead : MicroLead{};
    bool ok = true;
    pick<0, 1>(g_params != nullptr, [&](auto pv) {
        constexpr bool kParams = decltype(pv)::value != 0;
        const size_t lds = micro_ckpt_bwd_lds_bytes(V, S, kParams, target);
        if (f.kind == kObserveHist)
            ok = launch_lds(micro_rollout_ckpt_bwd_kernel<kParams>, L, pl.ckpt_block, lds, kLdsDefault, stream, L, V, T, S, d->dt, ck, count,
                            params, head, g_p, g_v, f.g_obs, g_p_out, g_v_out, g_head, g_params, err);
        else pick<0, 1, 2>(micro_form_boundary(f), [&](auto bv) {
            constexpr MicroBoundary kB = (MicroBoundary) decltype(bv)::value;
            if (f.kind == kObserveSamples)
                ok = launch_lds(micro_rollout_ckpt_bwd_samples_kernel<kParams, kB>, L, pl.ckpt_block, lds, kLdsDefault, stream, L, V, T, S,
                                d->dt, ck, count, params, head, g_p, g_v, f.pr, f.g_obs, g_p_out, g_v_out, g_head, g_params, err, ld);
            else
                ok = launch_lds(micro_rollout_ckpt_bwd_target_kernel<kParams, kB>, L, pl.ckpt_block, lds, kLdsDefault, stream, L, V, T, S,
                                d->dt, ck, count, params, head, g_p, g_v, f.target, f.g_sse, g_p_out, g_v_out, g_head, g_params, err, ld);
        });
    });
    return ok ? launch_status() : DHTS_E_LAUNCH;
}
template <bool kHeadOnly>
static int micro_step_tensor_launch(const dhts_micro_desc *d, const float *p, const float *v, const int32_t *count, const double *params,
                                    const double *head, float *p_out, float *v_out, float *tape, dhts_error *err, void *stream) {
    if (!micro_desc_ok(d) || !p || !v || !params || !head || !p_out || !v_out) return DHTS_E_INVALID;
    const int B = d->capacity <= 64 ? 64 : (d->capacity <= 128 ? 128 : 256);
    launch(micro_step_tensor_fwd_kernel<kHeadOnly>, d->n_lanes, B, 0, stream, d->n_lanes, d->capacity, d->dt, p, v, count, params, head,
           p_out, v_out, tape, err);
    return launch_status();
}

extern "C" {

int dhts_idm_batch(int64_t n, int variant, const double *in, double *next_pv, float *dEgo, float *dLeading, int32_t *collided,
                   double *acc_sstar, int32_t *clips, void *stream) {
    if (n < 0 || (variant != 0 && variant != 1) || !in || !next_pv || !dEgo || !dLeading || !collided || !acc_sstar || !clips) return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(idm_batch_kernel, grid_1d(n), 256, 0, stream, n, variant, in, next_pv, dEgo, dLeading, collided, acc_sstar, clips);
    return launch_status();
}

int dhts_idm_jac_batch(int64_t n, const double *in, float *dEgo, float *dLeading, void *stream) {
    if (n <= 0 || !in || !dEgo || !dLeading) return DHTS_E_INVALID;
    launch(idm_jac_batch_kernel, grid_1d(n, 4096), 256, 0, stream, n, in, dEgo, dLeading);
    return launch_status();
}

size_t dhts_micro_tape_bytes(const dhts_micro_desc *d, int T) {
    if (!micro_desc_ok(d) || T < 0) return 0;
    return (size_t)T * d->n_lanes * padded64(d->capacity) * sizeof(MicroTape3);
}
size_t dhts_micro_step_tape_bytes(const dhts_micro_desc *d) {
    if (!micro_desc_ok(d)) return 0;
    return (size_t)d->n_lanes * 2 * padded64(d->capacity) * sizeof(float4);
}

int dhts_micro_rollout_fwd(const dhts_micro_desc *d, int T,
                           const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                           float *p_out, float *v_out, float *tape, float *hist, dhts_error *err, void *stream) {
    return micro_fwd_launch<true>(d, T, p, v, count, params, head, p_out, v_out, tape, hist, err, stream);
}
int dhts_micro_rollout_bwd(const dhts_micro_desc *d, int T, const float *tape, const int32_t *count,
                                      const float *g_p, const float *g_v, const float *g_hist,
                                      float *g_p_out, float *g_v_out, double *g_head, dhts_error *err, void *stream) {
    return micro_bwd_launch<true>(d, T, tape, count, g_p, g_v, g_hist, g_p_out, g_v_out, g_head, 1, err, stream);
}
size_t dhts_micro_param_tape_bytes(const dhts_micro_desc *d, int T) {
    if (!micro_desc_ok(d) || T < 0) return 0;
    return param_tape_steps_offset(d->n_lanes) + (size_t)T * d->n_lanes * padded64(d->capacity) * micro_plan(d, T, false).ptape_bytes;
}
int dhts_micro_rollout_fwd_params(const dhts_micro_desc *d, int T,
                                  const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                                  float *p_out, float *v_out, float *tape, void *ptape, float *hist, dhts_error *err, void *stream) {
    return micro_fwd_launch<true, true>(d, T, p, v, count, params, head, p_out, v_out, tape, hist, err, stream, (char *)ptape);
}
int dhts_micro_rollout_bwd_params(const dhts_micro_desc *d, int T, const float *tape, const void *ptape, const int32_t *count,
                                  const double *params, const float *g_p, const float *g_v, const float *g_hist,
                                  float *g_p_out, float *g_v_out, double *g_head, double *g_params, dhts_error *err, void *stream) {
    return micro_bwd_params_launch(d, T, tape, (const char *)ptape, count, params, g_p, g_v, g_hist, g_p_out, g_v_out, g_head, g_params,
                                   err, stream);
}
int dhts_idm_param_jac_batch(int64_t n, const double *in, double *dacc, int32_t *clips, void *stream) {
    if (n <= 0 || !in || !dacc || !clips) return DHTS_E_INVALID;
    launch(idm_param_jac_batch_kernel, grid_1d(n, 4096), 256, 0, stream, n, in, dacc, clips);
    return launch_status();
}
// which kernel instantiations dhts_micro_rollout_fwd / _bwd launch for this shape: the plan the launches read
int dhts_micro_rollout_plan(const dhts_micro_desc *d, int T, int has_count, int32_t plan[8]) {
    if (!micro_desc_ok(d) || T < 0 || !plan) return DHTS_E_INVALID;
    const MicroPlan pl = micro_plan(d, T, has_count != 0);
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = pl.W;
    plan[1] = pl.K;
    plan[2] = pl.full ? 1 : 0;
    plan[3] = pl.bwd_per_thread ? 1 : 0;
    plan[4] = pl.bwd_block;
    plan[5] = pl.ptape_bytes;
    plan[6] = pl.pbwd_block;
    return DHTS_OK;
}
// ---- the tangent sweep ----------------------------------------------------------------------------------------------------------
int dhts_micro_rollout_jvp(const dhts_micro_desc *d, int T, int n_dir, const float *tape, const void *ptape, const int32_t *count,
                           const double *params, const float *t_p, const float *t_v, const double *t_head, const double *t_params,
                           float *t_p_out, float *t_v_out, float *t_hist, dhts_error *err, void *stream) {
    if (!micro_desc_ok(d) || T < 0 || n_dir < 1 || (T > 0 && !tape) || !t_p || !t_v || !t_p_out || !t_v_out) return DHTS_E_INVALID;
    if ((ptape != nullptr) != (params != nullptr) || (ptape != nullptr) != (t_params != nullptr)) return DHTS_E_INVALID;     // the three go together
    return micro_jvp_launch(d, T, n_dir, tape, (const char *)ptape, count, params, t_p, t_v, t_head, t_params, t_p_out, t_v_out, t_hist, err,
                            stream);
}
int dhts_micro_jvp_plan(const dhts_micro_desc *d, int T, int n_dir, int want_params, int32_t plan[8]) {
    if (!micro_desc_ok(d) || T < 0 || n_dir < 1 || !plan) return DHTS_E_INVALID;
    const MicroPlan pl = micro_plan(d, T, false);
    const JvpGroups g = jvp_groups(pl.jvp_kmax, n_dir);
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = pl.jvp_block;
    plan[1] = g.widest;
    plan[2] = g.launches;
    plan[3] = (int32_t)micro_jvp_lds_bytes(d->capacity, g.widest, want_params != 0);
    return DHTS_OK;
}
// ---- the rollout and its tangents in one kernel, no tape ------------------------------------------------------------------------
int dhts_micro_rollout_fwd_jvp(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                               const double *params, const double *head, const float *t_p, const float *t_v, const double *t_head,
                               const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out, float *hist,
                               float *t_hist, dhts_error *err, dhts_error *err_jvp, void *stream) {
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !micro_tangent_args_ok(n_dir, t_p, t_v, t_p_out, t_v_out) || !head)
        return DHTS_E_INVALID;
    return micro_fwd_jvp_launch(d, T, n_dir, p, v, count, params, head, t_p, t_v, t_head, t_params, p_out, v_out, t_p_out, t_v_out,
                                micro_form_hist(hist, t_hist, nullptr), err, err_jvp, stream);
}
int dhts_micro_fwd_jvp_plan(const dhts_micro_desc *d, int T, int n_dir, int want_params, int32_t plan[8]) {
    if (!micro_desc_ok(d) || T < 0 || n_dir < 1 || !plan) return DHTS_E_INVALID;
    const MicroPlan pl = micro_plan(d, T, false);
    const JvpGroups g = jvp_groups(pl.fwd_jvp_kmax[want_params != 0 ? 1 : 0], n_dir);
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = pl.fwd_jvp_block;
    plan[1] = g.widest;
    plan[2] = g.launches;
    plan[3] = (int32_t)micro_fwd_jvp_lds_bytes(d->capacity, g.widest);
    return DHTS_OK;
}
// ---- the Gauss-Newton normal equations of a trajectory fit inside the fused kernel ---------------------------------------------------
int dhts_micro_rollout_fwd_jvp_gn(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                  const double *params, const double *head, const float *lead, const double *lead_length,
                                  const double *ring, const float *t_p, const float *t_v, const double *t_head, const float *t_lead,
                                  const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                  const int32_t *probes, int n_probes, int every, const float *target, double *sse, double *jtr,
                                  double *jtj, dhts_error *err, dhts_error *err_jvp, void *stream) {
    MicroProbes pr;
    // the head follows exactly one of head, lead, ring (T = 0 reads no row of lead: a NULL lead is then the lead form's, as its siblings')
    const int bounds = (head != nullptr) + (lead != nullptr) + (ring != nullptr);
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !micro_tangent_args_ok(n_dir, t_p, t_v, t_p_out, t_v_out) ||
        bounds > 1 || (bounds == 0 && T > 0) || (t_head && !head) || ((t_lead || lead_length) && (head || ring || (!lead && T > 0))) ||
        !micro_probes_ok(d, probes, n_probes, every, &pr) || (T / every > 0 && !target) || !sse || !jtr || !jtj)
        return DHTS_E_INVALID;
    if (micro_gn_each_launch(n_dir, micro_gn_kmax(d->capacity, t_params != nullptr), [](bool, int, const int *) { return true; }) == 0)
        return DHTS_E_INVALID;
    const MicroLead ld = {lead, lead_length, nullptr, t_lead, ring};
    return micro_fwd_jvp_gn_launch(d, T, n_dir, p, v, count, params, head, t_p, t_v, t_head, t_params, p_out, v_out, t_p_out, t_v_out, pr,
                                   head ? nullptr : &ld, target, sse, jtr, jtj, err, err_jvp, stream);
}
int dhts_micro_fwd_jvp_gn_plan(const dhts_micro_desc *d, int T, int n_dir, int want_params, int32_t plan[8]) {
    if (!micro_desc_ok(d) || T < 0 || n_dir < 1 || !plan) return DHTS_E_INVALID;
    const int width = micro_gn_kmax(d->capacity, want_params != 0);
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = padded64(d->capacity);
    plan[1] = width;
    plan[2] = micro_gn_each_launch(n_dir, width, [](bool, int, const int *) { return true; });
    const int widest = n_dir >= 3 && width >= 4 ? 4 : (n_dir >= 2 && width >= 2 ? 2 : 1);
    plan[3] = (int32_t)micro_fwd_jvp_lds_bytes(d->capacity, widest);
    plan[4] = n_dir <= width ? n_dir : width / 2;
    plan[5] = micro_gn_bound(widest, want_params != 0);
    return DHTS_OK;
}
// ---- reverse mode from checkpoints, the segment tape in LDS ----------------------------------------------------------------------
int dhts_micro_ckpt_plan(const dhts_micro_desc *d, int T, int want_params, int segment, int32_t plan[8]) {
    return micro_ckpt_plan_fill(d, T, want_params != 0, segment, false, plan);
}
size_t dhts_micro_ckpt_bytes(const dhts_micro_desc *d, int T, int segment) {
    if (!micro_desc_ok(d) || T < 0) return 0;
    const int S = micro_ckpt_segment(micro_plan(d, T, false).ckpt[0], segment, false);
    if (S < 0) return 0;
    return (size_t)micro_ckpt_count(T, S) * d->n_lanes * padded64(d->capacity) * sizeof(float2);
}
int dhts_micro_rollout_fwd_ckpt(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                const double *params, const double *head, float *p_out, float *v_out, void *ckpt, float *hist,
                                dhts_error *err, void *stream) {
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !head || (T > 0 && !ckpt)) return DHTS_E_INVALID;
    return micro_ckpt_fwd_launch(d, T, segment, p, v, count, params, head, p_out, v_out, ckpt, micro_form_hist(hist, nullptr, nullptr), err,
                                 stream);
}
int dhts_micro_rollout_bwd_ckpt(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count, const double *params,
                                const double *head, const float *g_p, const float *g_v, const float *g_hist, float *g_p_out,
                                float *g_v_out, double *g_head, double *g_params, dhts_error *err, void *stream) {
    if (!micro_bwd_args_ok(d, T, params, g_p, g_v, g_p_out, g_v_out) || (T > 0 && !ckpt) || !head) return DHTS_E_INVALID;
    return micro_ckpt_bwd_launch(d, T, segment, ckpt, count, params, head, g_p, g_v, g_p_out, g_v_out, g_head, g_params,
                                 micro_form_hist(nullptr, nullptr, g_hist), err, stream);
}
// ---- probe samples on the two tape-free paths --------------------------------------------------------------------------------------
int dhts_micro_rollout_fwd_ckpt_samples(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                        const double *params, const double *head, float *p_out, float *v_out, void *ckpt,
                                        const int32_t *probes, int n_probes, int every, float *samples, dhts_error *err, void *stream) {
    MicroProbes pr;
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !head || !micro_probes_ok(d, probes, n_probes, every, &pr) ||
        (T / every > 0 && !samples))
        return DHTS_E_INVALID;
    return micro_ckpt_fwd_launch(d, T, segment, p, v, count, params, head, p_out, v_out, ckpt,
                                 micro_form_samples(pr, samples, nullptr, nullptr, nullptr), err, stream);
}
int dhts_micro_rollout_bwd_ckpt_samples(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                        const double *params, const double *head, const float *g_p, const float *g_v, const int32_t *probes,
                                        int n_probes, int every, const float *g_samples, float *g_p_out, float *g_v_out, double *g_head,
                                        double *g_params, dhts_error *err, void *stream) {
    MicroProbes pr;
    if (!micro_bwd_args_ok(d, T, params, g_p, g_v, g_p_out, g_v_out) || (T > 0 && !ckpt) || !head ||
        !micro_probes_ok(d, probes, n_probes, every, &pr) || (T / every > 0 && !g_samples))
        return DHTS_E_INVALID;
    return micro_ckpt_bwd_launch(d, T, segment, ckpt, count, params, head, g_p, g_v, g_p_out, g_v_out, g_head, g_params,
                                 micro_form_samples(pr, nullptr, nullptr, g_samples, nullptr), err, stream);
}
int dhts_micro_rollout_fwd_jvp_samples(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                       const double *params, const double *head, const float *t_p, const float *t_v, const double *t_head,
                                       const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                       const int32_t *probes, int n_probes, int every, float *samples, float *t_samples, dhts_error *err,
                                       dhts_error *err_jvp, void *stream) {
    MicroProbes pr;
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !micro_tangent_args_ok(n_dir, t_p, t_v, t_p_out, t_v_out) || !head ||
        !micro_probes_ok(d, probes, n_probes, every, &pr) || (T / every > 0 && (!samples || !t_samples)))
        return DHTS_E_INVALID;
    return micro_fwd_jvp_launch(d, T, n_dir, p, v, count, params, head, t_p, t_v, t_head, t_params, p_out, v_out, t_p_out, t_v_out,
                                micro_form_samples(pr, samples, t_samples, nullptr, nullptr), err, err_jvp, stream);
}
// ---- a recorded leader on the two tape-free paths: the kLead forms of the three sampled kernels ---------------------------------------
int dhts_micro_rollout_fwd_ckpt_lead(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                     const double *params, const float *lead, const double *lead_length, float *p_out, float *v_out,
                                     void *ckpt, const int32_t *probes, int n_probes, int every, float *samples, dhts_error *err,
                                     void *stream) {
    MicroProbes pr;
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || (T > 0 && !lead) || !micro_probes_ok(d, probes, n_probes, every, &pr))
        return DHTS_E_INVALID;
    const MicroLead ld = {lead, lead_length, nullptr, nullptr};
    return micro_ckpt_fwd_launch(d, T, segment, p, v, count, params, nullptr, p_out, v_out, ckpt,
                                 micro_form_samples(pr, samples, nullptr, nullptr, &ld), err, stream);
}
int dhts_micro_rollout_bwd_ckpt_lead(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                     const double *params, const float *lead, const double *lead_length, const float *g_p, const float *g_v,
                                     const int32_t *probes, int n_probes, int every, const float *g_samples, float *g_p_out, float *g_v_out,
                                     float *g_lead, double *g_params, dhts_error *err, void *stream) {
    MicroProbes pr;
    if (!micro_bwd_args_ok(d, T, params, g_p, g_v, g_p_out, g_v_out) || (T > 0 && (!ckpt || !lead || !g_lead)) ||
        !micro_probes_ok(d, probes, n_probes, every, &pr))
        return DHTS_E_INVALID;
    const MicroLead ld = {lead, lead_length, g_lead, nullptr};
    return micro_ckpt_bwd_launch(d, T, segment, ckpt, count, params, nullptr, g_p, g_v, g_p_out, g_v_out, nullptr, g_params,
                                 micro_form_samples(pr, nullptr, nullptr, g_samples, &ld), err, stream);
}
// ---- the trajectory-fit loss inside the checkpointed pair: the kTarget forms ------------------------------------------------------------
int dhts_micro_ckpt_target_plan(const dhts_micro_desc *d, int T, int want_params, int segment, int32_t plan[8]) {
    return micro_ckpt_plan_fill(d, T, want_params != 0, segment, true, plan);
}
int dhts_micro_rollout_fwd_ckpt_target(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                       const double *params, const double *head, const float *lead, const double *lead_length,
                                       float *p_out, float *v_out, void *ckpt, const float *target, double *sse, dhts_error *err,
                                       void *stream) {
    // head or lead, exactly one; T = 0 reads no row of lead, and a NULL lead is then accepted as dhts_micro_rollout_fwd_ckpt_lead accepts it
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || (head && (lead || lead_length)) || (!head && !lead && T > 0) ||
        (T > 0 && !target) || !sse)
        return DHTS_E_INVALID;
    const MicroLead ld = {lead, lead_length, nullptr, nullptr};
    return micro_ckpt_fwd_launch(d, T, segment, p, v, count, params, head, p_out, v_out, ckpt,
                                 micro_form_target(target, sse, nullptr, head ? nullptr : &ld), err, stream);
}
int dhts_micro_rollout_bwd_ckpt_target(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                       const double *params, const double *head, const float *lead, const double *lead_length,
                                       const float *g_p, const float *g_v, const float *target, const double *g_sse, float *g_p_out,
                                       float *g_v_out, double *g_head, float *g_lead, double *g_params, dhts_error *err, void *stream) {
    if (!micro_bwd_args_ok(d, T, params, g_p, g_v, g_p_out, g_v_out) || (T > 0 && (!ckpt || !target)) ||
        (head && (lead || lead_length || g_lead)) || (!head && (g_head || (T > 0 && (!lead || !g_lead)))))
        return DHTS_E_INVALID;
    const MicroLead ld = {lead, lead_length, g_lead, nullptr};
    return micro_ckpt_bwd_launch(d, T, segment, ckpt, count, params, head, g_p, g_v, g_p_out, g_v_out, g_head, g_params,
                                 micro_form_target(target, nullptr, g_sse, head ? nullptr : &ld), err, stream);
}
int dhts_micro_rollout_fwd_jvp_lead(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                    const double *params, const float *lead, const double *lead_length, const float *t_p, const float *t_v,
                                    const float *t_lead, const double *t_params, float *p_out, float *v_out, float *t_p_out, float *t_v_out,
                                    const int32_t *probes, int n_probes, int every, float *samples, float *t_samples, dhts_error *err,
                                    dhts_error *err_jvp, void *stream) {
    MicroProbes pr;
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !micro_tangent_args_ok(n_dir, t_p, t_v, t_p_out, t_v_out) ||
        (T > 0 && !lead) || !micro_probes_ok(d, probes, n_probes, every, &pr) || (samples == nullptr) != (t_samples == nullptr))
        return DHTS_E_INVALID;
    const MicroLead ld = {lead, lead_length, nullptr, t_lead};
    return micro_fwd_jvp_launch(d, T, n_dir, p, v, count, params, nullptr, t_p, t_v, nullptr, t_params, p_out, v_out, t_p_out, t_v_out,
                                micro_form_samples(pr, samples, t_samples, nullptr, &ld), err, err_jvp, stream);
}
// ---- a ring road on the two tape-free paths: the kBoundRing forms of the three sampled and the two target kernels ------------------------
// (ring is read by the kernels once per lane; head, lead and every cotangent or tangent of them do not exist)
int dhts_micro_rollout_fwd_ckpt_ring(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v, const int32_t *count,
                                     const double *params, const double *ring, float *p_out, float *v_out, void *ckpt,
                                     const int32_t *probes, int n_probes, int every, float *samples, dhts_error *err, void *stream) {
    MicroProbes pr;
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !ring || !micro_probes_ok(d, probes, n_probes, every, &pr))
        return DHTS_E_INVALID;
    const MicroLead ld = {nullptr, nullptr, nullptr, nullptr, ring};
    return micro_ckpt_fwd_launch(d, T, segment, p, v, count, params, nullptr, p_out, v_out, ckpt,
                                 micro_form_samples(pr, samples, nullptr, nullptr, &ld), err, stream);
}
int dhts_micro_rollout_bwd_ckpt_ring(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                     const double *params, const double *ring, const float *g_p, const float *g_v, const int32_t *probes,
                                     int n_probes, int every, const float *g_samples, float *g_p_out, float *g_v_out, double *g_params,
                                     dhts_error *err, void *stream) {
    MicroProbes pr;
    if (!micro_bwd_args_ok(d, T, params, g_p, g_v, g_p_out, g_v_out) || (T > 0 && !ckpt) || !ring ||
        !micro_probes_ok(d, probes, n_probes, every, &pr))
        return DHTS_E_INVALID;
    const MicroLead ld = {nullptr, nullptr, nullptr, nullptr, ring};
    return micro_ckpt_bwd_launch(d, T, segment, ckpt, count, params, nullptr, g_p, g_v, g_p_out, g_v_out, nullptr, g_params,
                                 micro_form_samples(pr, nullptr, nullptr, g_samples, &ld), err, stream);
}
int dhts_micro_rollout_fwd_jvp_ring(const dhts_micro_desc *d, int T, int n_dir, const float *p, const float *v, const int32_t *count,
                                    const double *params, const double *ring, const float *t_p, const float *t_v, const double *t_params,
                                    float *p_out, float *v_out, float *t_p_out, float *t_v_out, const int32_t *probes, int n_probes,
                                    int every, float *samples, float *t_samples, dhts_error *err, dhts_error *err_jvp, void *stream) {
    MicroProbes pr;
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !micro_tangent_args_ok(n_dir, t_p, t_v, t_p_out, t_v_out) || !ring ||
        !micro_probes_ok(d, probes, n_probes, every, &pr) || (samples == nullptr) != (t_samples == nullptr))
        return DHTS_E_INVALID;
    const MicroLead ld = {nullptr, nullptr, nullptr, nullptr, ring};
    return micro_fwd_jvp_launch(d, T, n_dir, p, v, count, params, nullptr, t_p, t_v, nullptr, t_params, p_out, v_out, t_p_out, t_v_out,
                                micro_form_samples(pr, samples, t_samples, nullptr, &ld), err, err_jvp, stream);
}
int dhts_micro_rollout_fwd_ckpt_target_ring(const dhts_micro_desc *d, int T, int segment, const float *p, const float *v,
                                            const int32_t *count, const double *params, const double *ring, float *p_out, float *v_out,
                                            void *ckpt, const float *target, double *sse, dhts_error *err, void *stream) {
    if (!micro_fwd_args_ok(d, T, p, v, params, p_out, v_out) || !ring || (T > 0 && !target) || !sse) return DHTS_E_INVALID;
    const MicroLead ld = {nullptr, nullptr, nullptr, nullptr, ring};
    return micro_ckpt_fwd_launch(d, T, segment, p, v, count, params, nullptr, p_out, v_out, ckpt, micro_form_target(target, sse, nullptr, &ld),
                                 err, stream);
}
int dhts_micro_rollout_bwd_ckpt_target_ring(const dhts_micro_desc *d, int T, int segment, const void *ckpt, const int32_t *count,
                                            const double *params, const double *ring, const float *g_p, const float *g_v,
                                            const float *target, const double *g_sse, float *g_p_out, float *g_v_out, double *g_params,
                                            dhts_error *err, void *stream) {
    if (!micro_bwd_args_ok(d, T, params, g_p, g_v, g_p_out, g_v_out) || (T > 0 && (!ckpt || !target)) || !ring) return DHTS_E_INVALID;
    const MicroLead ld = {nullptr, nullptr, nullptr, nullptr, ring};
    return micro_ckpt_bwd_launch(d, T, segment, ckpt, count, params, nullptr, g_p, g_v, g_p_out, g_v_out, nullptr, g_params,
                                 micro_form_target(target, nullptr, g_sse, &ld), err, stream);
}
// the single-step operator keeps the reference's dqs[a][2][2][2] (32 B per vehicle)
int dhts_micro_step_fwd(const dhts_micro_desc *d,
                        const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                        float *p_out, float *v_out, float *tape, dhts_error *err, void *stream) {
    return micro_fwd_launch<false>(d, 1, p, v, count, params, head, p_out, v_out, tape, nullptr, err, stream);
}
int dhts_micro_step_fwd_tensor(const dhts_micro_desc *d,
                               const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                               float *p_out, float *v_out, float *tape, dhts_error *err, void *stream) {
    return micro_step_tensor_launch<false>(d, p, v, count, params, head, p_out, v_out, tape, err, stream);
}
int dhts_micro_step_fwd_tensor_head(const dhts_micro_desc *d,
                                    const float *p, const float *v, const int32_t *count, const double *params, const double *head,
                                    float *p_out, float *v_out, float *tape, dhts_error *err, void *stream) {
    return micro_step_tensor_launch<true>(d, p, v, count, params, head, p_out, v_out, tape, err, stream);
}
int dhts_micro_step_bwd(const dhts_micro_desc *d, const float *tape, const int32_t *count,
                        const float *g_p, const float *g_v,
                        float *g_p_out, float *g_v_out, double *g_head, dhts_error *err, void *stream) {
    return micro_bwd_launch<false>(d, 1, tape, count, g_p, g_v, nullptr, g_p_out, g_v_out, g_head, 0, err, stream);
}

}  // extern "C"
