// macro_kernels.hip -- time-fused forward and reverse sweeps of the ARZ cell stencil on gfx950.
//
// Forward (macro_rollout_fwd_kernel): one workgroup of W wavefronts owns one traffic lane for the whole rollout.
//   The lane's state (r, y, u, u_eq; float32, N cells + 2 ghosts) lives in LDS (ping-pong) for all T steps; HBM
//   sees only the initial load, the final store and the Jacobian tape (48 B per cell-step, written as three
//   coalesced 16-B-per-lane streams).  Each wave owns a contiguous chunk of cells and walks it in 64-interface
//   passes: thread t of a pass solves ONE interface (between cells i-1 and i) once, hands the result to thread
//   t-1 with a DPP wave shift (the cell left of an interface needs it as ITS right interface), and thread 63
//   takes the first interface of the previous pass from scalar registers.  One workgroup barrier per time
//   step; no inter-workgroup traffic.
// Reverse (macro_rollout_bwd_kernel): one workgroup per lane, cotangent (g_r, g_y) in LDS, tape read back as the
//   same three streams, newest step first; g' = J^T g with the reference's float32 accumulation order.
//
// Reference: road/lane/_macro_lane.py:83-146, road/lane/dmacro_lane.py:96-132 and :277-309.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/dhts.h"
#include "arz_device.hpp"
#include "host_common.hpp"

namespace dhts {

// wave_shl:1 DPP move: lane t receives lane t+1's value; lane 63 (no source) keeps `carry`.
// One v_mov_b32_dpp per dword -- no LDS round trip.
constexpr int kDppWaveShl1 = 0x130;
__device__ __forceinline__ float take_right(float x, float carry) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(carry), __float_as_int(x), kDppWaveShl1, 0xF, 0xF, false));
}
__device__ __forceinline__ unsigned take_right(unsigned x, unsigned carry) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)carry, (int)x, kDppWaveShl1, 0xF, 0xF, false);
}
__device__ __forceinline__ double take_right(double x, double carry) {
    const long long xb = __double_as_longlong(x), cb = __double_as_longlong(carry);
    const int lo = __builtin_amdgcn_update_dpp((int)(cb & 0xffffffffll), (int)(xb & 0xffffffffll), kDppWaveShl1, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(cb >> 32), (int)(xb >> 32), kDppWaveShl1, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ float bcast0(float x) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ double bcast0(double x) {
    long long b = __double_as_longlong(x);
    int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
    int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---- the rollout tape -----------------------------------------------------------------------------------------------
// What the reverse sweep needs of a step is, per interface i, A_i = flux'(Q_0) dQ_0/dQ_L and B_i = flux'(Q_0) dQ_0/dQ_R
// (dmacro_lane.py:116-124).  For a trivial interface (Q_0 = Q_L; 85-89 % of them in BASELINE config 2) dQ_0/dQ_L = I and
// dQ_0/dQ_R = 0: A_i is the flux Jacobian at Q_L, whose entry [0][1] is the constant 1 (darz.py:217-233), and B_i = 0 --
// three floats instead of eight.  The other interfaces ("exceptions") keep their (A, B), compacted in the order the forward
// solved them.  One row per (step, lane), every block on a 128-byte line:
//   S  float [N][3]                                fp[0], fp[2], fp[3] of interface i < N where it is trivial
//   H  u32 cnt, u32 0 | u16 idx [N + 1]            idx[j] = interface of exception j < cnt; interface N is always one
//   E  float4 [N + 1][2]                           (A, B) of exception j; only the first cnt entries are written / read
// 8.8 KB of traffic per 512-cell row against the 16.6 KB of a dense (A, B) tape and the 24.6 KB of the reference's blocks.
struct TapeGeom {
    int s_f4, h_f4, e_f4;
    size_t row_f4;
};
__host__ __device__ inline TapeGeom tape_geom(int N) {
    TapeGeom g;
    g.s_f4 = (((3 * N + 3) >> 2) + 7) & ~7;
    g.h_f4 = ((8 + 2 * (N + 1) + 127) >> 7) << 3;
    g.e_f4 = (2 * (N + 1) + 7) & ~7;
    g.row_f4 = (size_t)g.s_f4 + g.h_f4 + g.e_f4;
    return g;
}
__device__ __forceinline__ unsigned *tape_hdr(float4 *row, const TapeGeom &g) { return reinterpret_cast<unsigned *>(row + g.s_f4); }
__device__ __forceinline__ const unsigned *tape_hdr(const float4 *row, const TapeGeom &g) { return reinterpret_cast<const unsigned *>(row + g.s_f4); }
__device__ __forceinline__ unsigned short *tape_idx(unsigned *hdr, const TapeGeom &g) { return reinterpret_cast<unsigned short *>(hdr + 2); }
__device__ __forceinline__ const unsigned short *tape_idx(const unsigned *hdr, const TapeGeom &g) { return reinterpret_cast<const unsigned short *>(hdr + 2); }
struct __attribute__((packed, aligned(4))) TapeFp { float f0, f2, f3; };
static_assert(sizeof(TapeFp) == 12, "TapeFp layout");
// (the lane kernels write it member by member through a plain pointer -- measured in round 2 against three planes, 4.32 against
// 4.44 ms; the pair kernel stores it as ONE 12-byte buffer store through the step's row descriptor: fp_tape_bits below)
typedef unsigned bits3 __attribute__((ext_vector_type(3)));      // what the 12- and 16-byte buffer loads and stores carry
typedef unsigned bits4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bits3 fp_tape_bits(const TapeFp &f) { return bits3{__float_as_uint(f.f0), __float_as_uint(f.f2), __float_as_uint(f.f3)}; }
__device__ __forceinline__ bits4 bits_f4(float a, float b, float c, float d) { return bits4{__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)}; }
__device__ __forceinline__ float4 tape_trivial_A(const TapeFp &s) { return make_float4(s.f0, 1.f, s.f2, s.f3); }

// ---- detector taps (dhts_macro_rollout_fwd_taps) -------------------------------------------------------------------
// kTaps in the forward kernels: `taps` [T][L][3][n_det] receives (r, y, u) of the cells det[0 .. n_det) after every step -- what
// hist[t][l][:][det[j]] would hold -- without a history.  MAPPING: the cell's owner does not store its own cell (it would carry a slot
// index per owned cell through the whole step loop: two registers in the pair kernel, which has six to spare under its 128); the reading
// threads do -- thread j' of the tap wavefronts takes detector j', keeps det[j'] in ONE register for the whole rollout and, behind the
// barrier that already orders the step's cell records (LDS) for phase 2, reads the record of that cell and stores its three floats.
// The tap wavefronts are the LAST ones of a lane (the first ones hold the head of the phase-2 queue); a wavefront whose first detector
// slot is >= n_det pays one scalar branch per step.  The final step writes no records (nothing solves after it): the taps forms store
// the float32 state once more and take one extra barrier, once per rollout, so that every row comes out of the same code.
// INDEX CONTRACT: det[] is not validated on the host (no sync).  An entry is compared against [0, N) as an unsigned value before any
// address is formed from it; an entry outside matches no cell and its column is not written.  j itself is a loop counter < n_det.
template <class RecAt>
__device__ __forceinline__ void taps_write(const int32_t *__restrict__ det, int n_det, int det_own, int j0, int stride, int N,
                                           float *__restrict__ row, RecAt rec_at) {
    for (int j = j0; j < n_det; j += stride) {
        const unsigned dc = (unsigned)(j == j0 ? det_own : det[j]);      // (detectors beyond one per thread: re-read, D > threads only)
        if (dc < (unsigned)N) {
            const float4 st = rec_at(dc);
            row[j] = st.x; row[n_det + j] = st.y; row[2 * n_det + j] = st.z;
        }
    }
}

// grid = L workgroups (one traffic lane each) of W = blockDim.x / 64 wavefronts; dynamic LDS = 2 * 4 * (N + 2) floats.
// Wave w owns the cells [w C, min(N, (w + 1) C)) with C = 64 p - 1, i.e. at most 64 p interfaces = p passes, so no
// wave ever needs a pass for a single left-over interface; the state is ping-pong buffered in LDS and the only
// synchronisation is one workgroup barrier per time step.
// kSched: `ghost` is a boundary schedule [T][L][2][4] (dhts_macro_rollout_fwd_sched): row 0 is loaded like a constant ghost; the row of
// step + 1 goes into the OTHER buffer's boundary slots at the end of step `step`, out of registers that were loaded one step earlier
// (threads 0 .. 7, one float each), so no step waits for the load it issues.
// kTaps: see above; the state after step `step` is the plane set the step wrote, which the next step only reads.
template <bool kIface, bool kSched = false, bool kTaps = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(5, 5))) void macro_rollout_fwd_kernel(
    int L, int N, int T, int p, double dt, double dx, double um,
    const float *__restrict__ r_in, const float *__restrict__ y_in, const float *__restrict__ u_in,
    const float *__restrict__ q_in, const float *__restrict__ ghost,
    float *__restrict__ r_out, float *__restrict__ y_out, float *__restrict__ u_out, float *__restrict__ q_out,
    float4 *__restrict__ tape, float *__restrict__ hist, dhts_error *err,
    const int32_t *__restrict__ det, int n_det, float *__restrict__ taps) {
    extern __shared__ float lds[];
    const int lane = blockIdx.x;
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int wv = tid >> 6;
    const int P = N + 2;
    int det_own = -1;
    if constexpr (kTaps) { if (tid < n_det) det_own = det[tid]; }
    const size_t base = (size_t)lane * N;

    // buffer b, plane k (r, y, u, u_eq) at lds + (b * 4 + k) * P; index c + 1 holds cell c, 0 and N + 1 the ghosts
    for (int k = tid; k < N; k += blockDim.x) {
        lds[0 * P + k + 1] = r_in[base + k];
        lds[1 * P + k + 1] = y_in[base + k];
        lds[2 * P + k + 1] = u_in[base + k];
        lds[3 * P + k + 1] = q_in[base + k];
    }
    if (tid < 16) {
        const int b = tid >> 3, side = (tid >> 2) & 1, k = tid & 3;
        lds[(b * 4 + k) * P + (side ? N + 1 : 0)] = ghost[(size_t)lane * 8 + side * 4 + k];
    }
    __syncthreads();

    const int C = 64 * p - 1;
    const int lo = wv * C;                           // first cell / first interface of this wave
    const int hi = (lo + C < N) ? lo + C : N;        // one past its last cell = its last interface
    const int K = (lo < N) ? ((hi - lo + 1 + 63) >> 6) : 0;
    const int Np = (N + 63) & ~63;
    const TapeGeom geo = tape_geom(N);
    const size_t tape_row = kIface ? geo.row_f4 : (size_t)3 * Np;
    const double c = dt / dx;                        // update_coefficient, _macro_lane.py:99
    const float cf = (float)c, ncf = (float)(-c);
    const float umf = (float)um;
    IfaceConst kc;
    kc.set_um(um); kc.set_grid(dt, dx);
    int fault_step = -1, fault_index = 0;
    // an upstream ghost in double (ghost_source_pack, arz_device.hpp: the itscp source lanes of the stepwise network paths)
    const bool src_ghost = !kSched && ghost_is_source(ghost[(size_t)lane * 8]);     // (a schedule holds float32 cells only)
    double src_r = 0., src_y = 0., src_u = 0., src_q = 0.;
    if (src_ghost) ghost_source_unpack(ghost[(size_t)lane * 8 + 2], ghost[(size_t)lane * 8 + 3], um, src_r, src_y, src_u, src_q);
    float sched_v = 0.f;                             // element (side, k) = (tid >> 2, tid & 3) of the next step's row
    const float *sched_p = nullptr;
    if constexpr (kSched) {
        sched_p = ghost + ((size_t)L + lane) * 8 + (tid & 7);
        if (tid < 8 && T > 1) sched_v = *sched_p;
    }

    for (int step = 0; step < T; ++step) {
        const float *cur = lds + (step & 1) * 4 * P;
        float *nxt = lds + ((step & 1) ^ 1) * 4 * P;
        const float *Sr = cur, *Sy = cur + P, *Su = cur + 2 * P, *Sq = cur + 3 * P;
        // first interface of the pass above (j + 1), broadcast from its thread 0
        double cFr = 0., cFy = 0.;
        float cA0 = 0.f, cA1 = 0.f, cA2 = 0.f, cA3 = 0.f, cB0 = 0.f, cB1 = 0.f, cB2 = 0.f, cB3 = 0.f;
        float4 *tp = tape ? tape + ((size_t)step * L + lane) * tape_row : nullptr;
        float *hp = hist ? hist + ((size_t)step * L + lane) * 3 * N : nullptr;
        if (kIface && tp) {
            // this kernel keeps every interface as an exception: interface N at slot 0, interface i < N at slot i + 1
            unsigned *H = tape_hdr(tp, geo);
            if (tid == 0) { H[0] = (unsigned)(N + 1); H[1] = 0u; }
        }
        if (K > 0) {
            for (int j = K - 1; j >= 0; --j) {
                const int i = lo + (j << 6) + t;   // interface i, and cell i to its right
                const bool vi = i <= hi;
                const bool vc = i < hi;
                const int ip = vi ? i : hi;
                double rL = Sr[ip], yL = Sy[ip], uL = Su[ip], qL = Sq[ip];
                if (src_ghost && ip == 0) { rL = src_r; yL = src_y; uL = src_u; qL = src_q; }
                const double rR = Sr[ip + 1], yR = Sy[ip + 1], uR = Su[ip + 1], qR = Sq[ip + 1];
                Iface f;
                arz_interface(rL, yL, uL, qL, rR, yR, uR, qR, kc, f);
                // CFL: dt < dx / max(|speed|, 1e-5) for both speeds (_macro_lane.py:141-146)
                if (vi && fault_step < 0 && f.cfl_bad) { fault_step = step; fault_index = i; }

                // right interface of cell i = interface i + 1: thread t + 1, or the carried one for thread 63
                const double Fr_R = take_right(f.Fr, cFr), Fy_R = take_right(f.Fy, cFy);
                cFr = bcast0(f.Fr); cFy = bcast0(f.Fy);
                float A0 = 0.f, A1 = 0.f, A2 = 0.f, A3 = 0.f, B0 = 0.f, B1 = 0.f, B2 = 0.f, B3 = 0.f;
                if constexpr (!kIface) {
                    A0 = take_right(f.A[0], cA0); A1 = take_right(f.A[1], cA1);
                    A2 = take_right(f.A[2], cA2); A3 = take_right(f.A[3], cA3);
                    B0 = take_right(f.B[0], cB0); B1 = take_right(f.B[1], cB1);
                    B2 = take_right(f.B[2], cB2); B3 = take_right(f.B[3], cB3);
                    cA0 = bcast0(f.A[0]); cA1 = bcast0(f.A[1]); cA2 = bcast0(f.A[2]); cA3 = bcast0(f.A[3]);
                    cB0 = bcast0(f.B[0]); cB1 = bcast0(f.B[1]); cB2 = bcast0(f.B[2]); cB3 = bcast0(f.B[3]);
                } else if (tp && vi) {
                    // the two 2x2 products of interface i; the reverse sweep forms the cell blocks from them
                    const int slot = (i == N) ? 0 : i + 1;
                    float4 *E = tp + geo.s_f4 + geo.h_f4;
                    E[2 * slot] = make_float4(f.A[0], f.A[1], f.A[2], f.A[3]);
                    E[2 * slot + 1] = make_float4(f.B[0], f.B[1], f.B[2], f.B[3]);
                    tape_idx(tape_hdr(tp, geo), geo)[slot] = (unsigned short)i;
                }

                if (vc) {
                    // Godunov update, _macro_lane.py:109-112, float32 store :327-334
                    const float nr = (float)(rR + (f.Fr - Fr_R) * c);
                    const float ny = (float)(yR + (f.Fy - Fy_R) * c);
                    float nu, nq;
                    glue_from_r_y(nr, ny, umf, nu, nq);      // set_next_state_vector_y, :282-299
                    nxt[i + 1] = nr; nxt[P + i + 1] = ny; nxt[2 * P + i + 1] = nu; nxt[3 * P + i + 1] = nq;
                    if (!kIface && tp) {
                        // dMacroLane._backward, dmacro_lane.py:126-129
                        float4 d0, d1, d2;
                        d0.x = ncf * (-f.A[0]); d0.y = ncf * (-f.A[1]); d0.z = ncf * (-f.A[2]); d0.w = ncf * (-f.A[3]);
                        d2.x = ncf * B0; d2.y = ncf * B1; d2.z = ncf * B2; d2.w = ncf * B3;
                        d1.x = 1.f - cf * (A0 - f.B[0]); d1.y = 0.f - cf * (A1 - f.B[1]);
                        d1.z = 0.f - cf * (A2 - f.B[2]); d1.w = 1.f - cf * (A3 - f.B[3]);
                        tp[i] = d0;
                        tp[Np + i] = d1;
                        tp[2 * Np + i] = d2;
                    }
                    if (hp) { hp[i] = nr; hp[N + i] = ny; hp[2 * N + i] = nu; }
                }
            }
        }
        if constexpr (kSched) {
            if (tid < 8 && step + 1 < T) {
                nxt[(tid & 3) * P + ((tid >> 2) ? N + 1 : 0)] = sched_v;
                sched_p += (size_t)L * 8;
                if (step + 2 < T) sched_v = *sched_p;
            }
        }
        __syncthreads();
        if constexpr (kTaps) {
            if (__builtin_amdgcn_readfirstlane(wv << 6) < n_det) {
                const float *nx = nxt;
                taps_write(det, n_det, det_own, tid, (int)blockDim.x, N, taps + ((size_t)step * L + lane) * 3 * n_det, [=](unsigned dc) {
                    return make_float4(nx[dc + 1], nx[P + dc + 1], nx[2 * P + dc + 1], 0.f);
                });
            }
        }
    }
    const float *fin = lds + (T & 1) * 4 * P;
    for (int k = tid; k < N; k += blockDim.x) {
        r_out[base + k] = fin[k + 1];
        y_out[base + k] = fin[P + k + 1];
        u_out[base + k] = fin[2 * P + k + 1];
        q_out[base + k] = fin[3 * P + k + 1];
    }
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_CFL, fault_step, lane, fault_index);
}

// ---- the rollout forward kernel: cheap solve everywhere, full solve only where needed ---------------------------------
__device__ __forceinline__ void lds_only_barrier() {     // global stores (the tape) stay in flight across it
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// Orders this wavefront's LDS stores in front of its later LDS loads FOR THE COMPILER: lanes of one wavefront hand data to
// each other through LDS (a cell's record to its right neighbour's thread, a pass's records and fluxes to the next pass), and
// within one thread those addresses never alias, so nothing else stops the scheduler from hoisting the loads.  The hardware
// executes a wavefront's LDS operations in order; no instruction is emitted.
__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One cell's record in LDS (48 bytes; a 48-byte stride keeps 16-byte accesses of 16 consecutive lanes on distinct banks):
// the float32 state and what the interface to the cell's right needs of it, computed once by the cell's owner.
struct __attribute__((aligned(16))) CellRec {
    float4 st;       // r, y, u, u_eq  (FullQ, _arz.py:10-115)
    double2 sh;      // CellPre s, h
    double2 q0;      // CellPre q0 (+ padding: every access is a conflict-free 16-byte one).  The padding q0.y is read by no step; the
                     // checkpointed reverse kernel's ramp forms keep the cell's ramp column in its first four bytes (ramp_col_get / _set,
                     // macro_ckpt.inc) and write q0.x alone
};
static_assert(sizeof(CellRec) == 48, "CellRec layout");

// New (u, u_eq) of a cell from its new (r, y) -- FullQ.set_r_y, _arz.py:88-92, float32 torch arithmetic -- together with
// the cell's CellPre.  The float32 square root and division of the glue come out of the double-precision square roots
// CellPre needs anyway: sqrtf(t32) = fl32(sE + (t32 - tE) hE) with sE = sqrt(tE), hE = 0.5 / sE, tE = r + eps in double
// (first-order in t32 - tE = O(1e-7): the remainder is 5e-16 relative), y / r = fl32(y (2 h)^2).  Both agree with the
// correctly rounded float32 result unless it lies within 2e-14 (relative) of a rounding boundary, i.e. except with
// probability ~1e-6 per operation -- the level of the fast double layer (fast_math.hpp); the IEEE forms are glue_from_r_y.
__device__ __forceinline__ void cell_glue_pre(float r, float y, float umf, const IfaceConst &k, float &u, float &q, CellPre &c) {
    const double rd = (double)r;
    sqrt_hrsqrt(fmax(rd, kEps), c.s, c.h);
    const double tE = fmax(rd, 0.) + kEps;
    double sE, hE;
    sqrt_hrsqrt(tE, sE, hE);
    c.q0 = __builtin_fma(-k.um, sE, k.um);
    const float t32 = r + kEpsF;
    const float s32 = (float)__builtin_fma((double)t32 - tE, hE, sE);
    const float one_m = 1.f - s32;
    q = (0.f > r) ? k.ueq_neg_f : umf * one_m;              // max(r, 0.) picked the Python float 0. (glue_u_eq)
    const double rs = c.h + c.h;
    const double inv = (r <= kEpsF) ? k.inv_epsf : rs * rs;  // 1 / max(r, eps32): r below OR AT float32(eps) divides by float32(eps)
    const float yor = (float)((double)y * inv);
    u = yor + ((r < kEpsF) ? k.ueq_2eps_f : q);
}

// grid = L workgroups (one traffic lane each) of W = blockDim.x / 64 wavefronts; wave w owns the cells [64 p w, 64 p (w + 1)),
// thread t of its pass j the cell c = 64 p w + 64 j + t and that cell's LEFT interface (interface c, between cells c-1 and c).
// In BASELINE config 2, 89 % of the interface solves end in the trivial case (Q_0 = Q_L, dQ_0/dQ_L = I, dQ_0/dQ_R = 0), but
// a 64-wide pass is uniformly trivial only 23 % of the time: evaluated in place, the Q_M / Q_C states with their Jacobians
// (more than half of the work) are paid for by every lane.  And on this chip every vector instruction of a wavefront costs
// about 4 cycles whatever its type (PMC: profiles/r02*), so the instruction COUNT is what a step costs, and the chain
// phase 1 -> phase 2 -> phase 1 ... of ONE lane is what bounds it when few lanes share a CU.  A step therefore runs as
//   phase 1 (every cell's thread): finish the previous step -- new (r, y) from the two fluxes of the cell, (u, u_eq) and
//     the cell's CellPre from one pair of square roots, written to the cell's record -- then read the left neighbour's
//     record, decide whether the interface is trivial, and if so write its flux (LDS) -- its tape entry is the three
//     non-constant entries of the flux Jacobian; otherwise append it to the lane's queue;
//   phase 2 (the first threads of the workgroup, one queue entry each, at raised priority: they are the workgroup's
//     critical path): the full solve for the queued interfaces, their fluxes to LDS, their tape entries to HBM.  Always
//     queued: the first interface of every wave's chunk (its left cell belongs to another wave) and interface N (no cell
//     owns it).
// One queue pass serves the whole lane (8 passes of phase 1 at 512 cells), so the expensive path runs about once per 64
// non-trivial interfaces instead of once per 64 interfaces.  Two LDS-only barriers per step.
// Where the time went when a wavefront made one pass (s_memtime stamps, config 2, 8 waves per lane, 2 workgroups per CU,
// 4.4 ms): phase 1 ~2000 cycles (every SIMD busy: instruction throughput), phase 2 ~1800 cycles on the one or two waves that
// hold queue entries while the others wait -- a dependent chain (three LDS round trips, the classification, two rsq / rcp
// chains, the Jacobians), latency not instruction count -- and ~600 cycles of barrier skew.  Since then (3.4 ms): the scalar
// diet (running pointers, literal flags: every instruction of a wavefront, scalar ones included, takes a turn of its
// issue slot) and two unrolled passes per wavefront (two independent cells per thread to interleave; four-wave workgroups,
// all lanes of config 2 resident at once).  Measured and dropped (tools/probes/*.hip.txt; times against the kernel of their day):
//   * fluxes only in phase 2, Jacobians one step behind on another wave: the Jacobian chain is as long as the full solve,
//     so the phase does not get shorter; a fifth / ninth dedicated wavefront per workgroup costs a workgroup of occupancy;
//   * the solve cut into three roles (flux | A | B) on three waves side by side: every role still takes ~1700 cycles;
//   * 6 or 8 waves per SIMD (80 / 64 VGPRs): no gain / spills;
//   * dedicated solver wavefronts (4 cell waves x 2 passes + 4 solver waves; the flux in front of the barrier that releases
//     the next phase 1, the Jacobians of the same entries behind it): 4.7 ms against 4.4 -- with half the waves owning
//     cells, phase 1 hides its own latency worse than phase 2 gets shorter; 8 + 4 waves need <= 80 VGPRs for two
//     workgroups per CU, which spills 35 registers;
//   * per-wave queues, every wave solving what it queued itself (no serial section, all waves busy in phase 2): 5.2 ms with
//     2 waves per lane, 5.9 with 8 -- the full solve's instruction stream is then paid once per wave instead of once per lane;
//   * the trivial interfaces' tape entries (three floats of the flux Jacobian) formed in phase 2 by the wavefronts that hold no
//     queue entry instead of in phase 1: 4.48 ms against 4.32 -- with two workgroups per CU those wavefronts are not idle
//     time, they are the other workgroup's phase 1;
//   * (round 3; all bitwise equal to the kernel below, gpurun_out/r03b_variants.log) the queue dealt round-robin over all four
//     wavefronts, 19 entries each, instead of 64 to the first and the rest to the second: 3.84 ms against 3.46 -- a wave
//     instruction costs its issue slot whatever its EXEC mask, so four wavefronts pay for the solve's stream instead of two;
//     phase 1 staged over both passes (every update, then every interface, then ONE queue append per wavefront): 3.50 --
//     the passes' streams interleave but the append was not what the wavefront waited for;
//   * two traffic lanes per workgroup half a step apart (phase 1 of one lane beside phase 2 of the other in every barrier
//     interval, 4 + 4 wavefronts, two phase-1 passes per thread interleaved stage by stage): 6.1 ms -- an interval takes
//     ~5100 cycles for the phase-1 waves and ~4000-4700 for the phase-2 waves that share their SIMDs, against 2000 + 1800
//     when the phases alternate: neither chain got shorter by running beside the other.
// Dynamic LDS: cell records [N + 2] (index c + 1 = cell c, 0 and N + 1 the ghosts; updated in place) | flux double2 [N + 1]
// | queue int [N + 2] | 2 counters.
// kP: 64-cell passes per wavefront as a literal (1 or 2; 0 = the run-time value p_arg): the pass loop is unrolled, the
// per-thread addresses are loop invariants, and with two passes a wavefront has two independent cells' instruction streams
// to interleave; kFull: every thread-pass owns a cell (N = kP blockDim.x): no validity masks; kHist: the state history may
// be asked for.  The step body is instantiated with literal (finish the previous step, start this one) flags: first step,
// steps in between, last.
// kSched: `ghost` is a boundary schedule [T][L][2][4]: threads 0 and 1 rewrite the two boundary records in phase 1 of every step n >= 1 (after
// the barrier behind phase 2 of step n - 1, the last reader of the old ones; thread 0, the only phase-1 reader, writes before it reads) from
// a row that has been in registers since step n - 1, then load the row of step n + 1.
// kTaps: detector taps (above), read in phase 2 of step n (state after step n - 1) from the records phase 1 has just written.
template <int kP, bool kFull, bool kHist, bool kSched = false, bool kTaps = false>
__global__ __launch_bounds__(1024) void macro_rollout_fwd2_kernel(
    int L, int N, int T, int p_arg, double dt, double dx, double um,
    const float *__restrict__ r_in, const float *__restrict__ y_in, const float *__restrict__ u_in,
    const float *__restrict__ q_in, const float *__restrict__ ghost,
    float *__restrict__ r_out, float *__restrict__ y_out, float *__restrict__ u_out, float *__restrict__ q_out,
    float4 *__restrict__ tape, float *__restrict__ hist, dhts_error *err,
    const int32_t *__restrict__ det, int n_det, float *__restrict__ taps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = blockIdx.x;
    const int tid = threadIdx.x;
    const int t = tid & 63;
    const int wv = tid >> 6;
    const int Wc = blockDim.x >> 6;                  // wavefronts
    const int ncell = blockDim.x;
    const size_t base = (size_t)lane * N;
    CellRec *CR = reinterpret_cast<CellRec *>(smem);
    double2 *FX = reinterpret_cast<double2 *>(CR + (N + 2));
    int *Q = reinterpret_cast<int *>(FX + (N + 1));
    int *CNT = Q + (N + 2);                          // queue length by step parity
    IfaceConst kc;
    kc.set_um(um); kc.set_grid(dt, dx);

    for (int k = tid; k < N + 2; k += blockDim.x) {
        float4 st;
        if (k == 0 || k == N + 1) {
            const float *g = ghost + (size_t)lane * 8 + (k ? 4 : 0);
            st = make_float4(g[0], g[1], g[2], g[3]);
        } else {
            st = make_float4(r_in[base + k - 1], y_in[base + k - 1], u_in[base + k - 1], q_in[base + k - 1]);
        }
        CellPre c;
        arz_cell_pre((double)st.x, um, c);
        CR[k].st = st;
        CR[k].sh = make_double2(c.s, c.h);
        CR[k].q0 = make_double2(c.q0, 0.);
    }
    if (tid == 0) { Q[0] = N; CNT[0] = 1; CNT[1] = 1; }      // entry 0 of every step's queue: interface N
    __syncthreads();

    const TapeGeom geo = tape_geom(N);
    const int p = kP > 0 ? kP : p_arg;

    const int lo = wv * (p << 6);                    // first cell of this wave
    const double c = dt / dx;                        // update_coefficient, _macro_lane.py:99
    const float umf = (float)um;
    int fault_step = -1, fault_index = 0;
    int rot = 0;                                     // the cell wave that takes the head of the queue rotates with the step

    // the tape row / history block of the step, advanced by one step's worth per trip (no 64-bit multiplications in the loop)
    float4 *tp_run = tape ? tape + (size_t)lane * geo.row_f4 : nullptr;
    float *hp_run = (kHist && hist) ? hist + (size_t)lane * 3 * N : nullptr;
    const size_t tp_stride = (size_t)L * geo.row_f4, hp_stride = (size_t)L * 3 * N;

    // (r, y) of a thread's own cells as doubles, carried from step to step: a thread owns the same cells for the whole rollout,
    // so the update neither re-reads them from the record nor widens them again (literal pass counts only; 3.46 -> 3.39 ms)
    constexpr bool kKeep = kP > 0;
    double rd_own[kP > 0 ? kP : 1], yd_own[kP > 0 ? kP : 1];

    float4 sched_st = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 *sched_p = nullptr;
    if constexpr (kSched) {
        sched_p = reinterpret_cast<const float4 *>(ghost) + ((size_t)L + lane) * 2 + (tid & 1);
        if (tid < 2 && T > 1) sched_st = *sched_p;
    }
    // kTaps: thread (blockDim - 1 - tid) takes detector slot tap_j (+ blockDim per further one); tap_wave: this wavefront holds any
    const int tap_j = (int)blockDim.x - 1 - tid;
    int det_own = -1;
    bool tap_wave = false;
    if constexpr (kTaps) {
        tap_wave = __builtin_amdgcn_readfirstlane((Wc - 1 - wv) << 6) < n_det;
        if (tap_j < n_det) det_own = det[tap_j];
    }
    auto tap = [&](const int s) {                       // the state after step s, out of the records
        if (tap_wave) {
            const CellRec *cr = CR;
            taps_write(det, n_det, det_own, tap_j, (int)blockDim.x, N, taps + ((size_t)s * L + lane) * 3 * n_det,
                       [=](unsigned dc) { return cr[dc + 1].st; });
        }
    };

    auto body = [&](auto upd_c, auto solve_c, const int n) {
        constexpr bool upd = decltype(upd_c)::value;       // finish step n - 1
        constexpr bool solve = decltype(solve_c)::value;   // start step n
        if constexpr (kSched && upd && solve) {
            if (tid < 2) {
                CellPre cg;
                arz_cell_pre((double)sched_st.x, um, cg);
                CellRec *gr = CR + (tid ? N + 1 : 0);
                gr->st = sched_st; gr->sh = make_double2(cg.s, cg.h); gr->q0 = make_double2(cg.q0, 0.);
                sched_p += (size_t)L * 2;
                if (n + 1 < T) sched_st = *sched_p;
            }
        }
        float4 *tp = solve ? tp_run : nullptr;
        TapeFp *tS = reinterpret_cast<TapeFp *>(tp);
        unsigned *tH = tape_hdr(tp, geo);
        float *hp = (kHist && upd) ? hp_run : nullptr;
        if (tp_run) tp_run += tp_stride;
        if (kHist && hp_run && upd) hp_run += hp_stride;
        int *cnt = CNT + (n & 1);
#pragma unroll
        for (int j = 0; j < p; ++j) {
            const int i = lo + (j << 6) + t;                // cell i and its left interface i
            const bool vc = kFull || i < N;
            const unsigned ic = (unsigned)(vc ? i : N - 1);
            CellRec *own = CR + ic + 1;
            float4 st;
            if (!(kKeep && upd)) st = own->st;
            if (kKeep && !upd) { rd_own[kP > 0 ? j : 0] = (double)st.x; yd_own[kP > 0 ? j : 0] = (double)st.y; }
            if (upd) {
                // Godunov update, _macro_lane.py:109-112, float32 store :327-334
                const double2 Fl = FX[ic], Fr = FX[ic + 1];
                const double r_old = kKeep ? rd_own[kP > 0 ? j : 0] : (double)st.x;
                const double y_old = kKeep ? yd_own[kP > 0 ? j : 0] : (double)st.y;
                st.x = (float)(r_old + (Fl.x - Fr.x) * c);
                st.y = (float)(y_old + (Fl.y - Fr.y) * c);
                if (kKeep) { rd_own[kP > 0 ? j : 0] = (double)st.x; yd_own[kP > 0 ? j : 0] = (double)st.y; }
                CellPre cp;
                cell_glue_pre(st.x, st.y, umf, kc, st.z, st.w, cp);     // set_next_state_vector_y, :282-299
                if (vc && solve) { own->st = st; own->sh = make_double2(cp.s, cp.h); own->q0 = make_double2(cp.q0, 0.); }
                else if (kTaps && vc) own->st = st;          // the final step's state, for the taps below
                if (vc && hp) { hp[i] = st.x; hp[N + i] = st.y; hp[2 * N + i] = st.z; }
            }
            if (!solve) {
                if (vc) { r_out[base + i] = st.x; y_out[base + i] = st.y; u_out[base + i] = st.z; q_out[base + i] = st.w; }
                continue;
            }
            // the left neighbour at this time level: written just above by the lane below, or in the previous pass (a wave's
            // LDS operations complete in order); the first cell of the chunk has its left neighbour in another wave: queued
            wave_lds_handoff();
            const CellRec *lf = CR + ic;
            const float4 ls = lf->st;
            const double2 lsh = lf->sh, lq0 = lf->q0;
            CellPre cl;
            cl.s = lsh.x; cl.h = lsh.y; cl.q0 = lq0.x;
            IfacePre pre;
            const bool easy = arz_is_trivial_fast((double)ls.x, (double)ls.z, (double)ls.w, (double)st.x, (double)st.z, cl, kc, pre);
            const bool triv = vc & easy & !((j == 0) & (t == 0));
            // the trivial solve runs on every lane (the few that are not trivial sit in the same instructions anyway); only
            // where it applies its flux counts.  Its flux Jacobian is the interface's tape entry.
            double u0, Fr, Fy;
            float fp[4];
            arz_trivial_fast((double)ls.x, (double)ls.y, pre, kc, u0, Fr, Fy, fp);
            if (triv) FX[ic] = make_double2(Fr, Fy);
            // append to the lane's queue: the compiler turns the per-lane atomic into ONE LDS atomic per wavefront (add of the
            // number of active lanes) and hands every lane the old value plus its rank among the active ones
            const bool nt = vc & !triv;
            if (nt) Q[atomicAdd(cnt, 1)] = i;
            if (tp && vc) tS[ic] = TapeFp{fp[0], fp[2], fp[3]};
        }
        if (!solve) {
            if constexpr (kTaps && upd) { lds_only_barrier(); tap(n - 1); }
            return;
        }
        lds_only_barrier();
        // ---- phase 2: the queued interfaces ----
        int k0 = tid - (rot << 6);
        if (k0 < 0) k0 += ncell;
        const unsigned i_q = (unsigned)Q[k0 <= N ? k0 : 0];  // read beside the count, not behind it (one LDS round trip less)
        const int qn = *cnt;
        if (k0 < qn) __builtin_amdgcn_s_setprio(3);          // the workgroup's critical path
        if (tp && k0 == 0) { tH[0] = (unsigned)qn; tH[1] = 0u; }
        float4 *tE = tp + geo.s_f4 + geo.h_f4;
        unsigned short *tI = tape_idx(tH, geo);
        for (int k = k0; k < qn; k += ncell) {
            const unsigned i = (k == k0) ? i_q : (unsigned)Q[k];
            const CellRec *lf = CR + i, *rt = CR + i + 1;
            const float4 ls = lf->st, rs = rt->st;
            const double2 lsh = lf->sh, lq0 = lf->q0, rsh = rt->sh;
            CellPre cl, cr;
            cl.s = lsh.x; cl.h = lsh.y; cl.q0 = lq0.x;
            cr.s = rsh.x; cr.h = rsh.y; cr.q0 = 0.;
            Iface f;
            arz_interface_fast_pre((double)ls.x, (double)ls.y, (double)ls.z, (double)ls.w, cl,
                                   (double)rs.x, (double)rs.y, (double)rs.z, (double)rs.w, cr, kc, f);
            FX[i] = make_double2(f.Fr, f.Fy);
            if (tp) {
                tE[2 * k] = make_float4(f.A[0], f.A[1], f.A[2], f.A[3]);
                tE[2 * k + 1] = make_float4(f.B[0], f.B[1], f.B[2], f.B[3]);
                tI[k] = (unsigned short)i;
            }
            if (f.cfl_bad && fault_step < 0) { fault_step = n; fault_index = (int)i; }
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (kTaps && upd) tap(n - 1);
        if (tid == 0) CNT[(n + 1) & 1] = 1;
        if (++rot == Wc) rot = 0;
        lds_only_barrier();
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;
    if (T == 0) {
        body(no{}, no{}, 0);
    } else {
        body(no{}, yes{}, 0);
        for (int n = 1; n < T; ++n) body(yes{}, yes{}, n);
        body(yes{}, no{}, T);
    }
    if (fault_step >= 0) raise_fault(err, DHTS_FAULT_CFL, fault_step, lane, fault_index);
}

// (Round 3's lane-group form of this kernel -- kG lanes per workgroup with one phase-2 list over their queues, 3.39 -> 3.22 ms at
// config 2 -- was what config 2 launched until the pair kernel of round 4 took every shape it covered; no plan selected it any more and
// it was removed in round 6.  docs/history/rounds_1-3_kernel_notebook.md keeps its measurements.)
#ifdef DHTS_FWD3_STAMPS
extern __device__ long long dhts_fwd_clock[2][16][2];     // macro_fwd_pairs.inc (instrumented builds only)
#endif

#include "macro_fwd_pairs.inc"

// ---- reverse sweeps -------------------------------------------------------------------------------------------------
// g' = J^T g per step: grad_cell[a][k] = dqs[a][k]^T g[a]; g'[b] = (c1[b] + c2[b-1]) + c0[b+1]   (dmacro_lane.py:283-303)
// LDS planes of (N + 2) floats: index k + 1 holds cell k; slots 0 and N + 1 stay zero for c2 / c0 so edge cells add 0.
struct BwdPlanes {
    float *Gr, *Gy, *C0r, *C0y, *C2r, *C2y;
};
__device__ __forceinline__ BwdPlanes bwd_planes(float *lds, int P) {
    return BwdPlanes{lds, lds + P, lds + 2 * P, lds + 3 * P, lds + 4 * P, lds + 5 * P};
}

// Reverse sweep over the single-step operator's blocked tape [lane][3][Np][4] (T = 1 from the C ABI; any T works).
// grid = L workgroups of `blockDim.x` threads (multiple of 64); dynamic LDS = 6 * (N + 2) floats.
__global__ void macro_blocks_bwd_kernel(
    int L, int N, int T, const float4 *__restrict__ tape,
    const float *__restrict__ g_r_in, const float *__restrict__ g_y_in, const float *__restrict__ g_hist,
    float *__restrict__ g_r_out, float *__restrict__ g_y_out, double *__restrict__ g_ghost, dhts_error *err) {
    extern __shared__ float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    const int B = blockDim.x;
    const int P = N + 2;
    const BwdPlanes pl = bwd_planes(lds, P);
    float *Gr = pl.Gr, *Gy = pl.Gy, *C0r = pl.C0r, *C0y = pl.C0y, *C2r = pl.C2r, *C2y = pl.C2y;
    const size_t base = (size_t)lane * N;
    const int Np = (N + 63) & ~63;
    const size_t tape_row = (size_t)3 * Np;

    for (int k = t; k < P; k += B) { C0r[k] = 0.f; C0y[k] = 0.f; C2r[k] = 0.f; C2y[k] = 0.f; Gr[k] = 0.f; Gy[k] = 0.f; }
    __syncthreads();
    for (int k = t; k < N; k += B) { Gr[k + 1] = g_r_in[base + k]; Gy[k + 1] = g_y_in[base + k]; }
    __syncthreads();

    double ghl_r = 0., ghl_y = 0., ghr_r = 0., ghr_y = 0.;   // ghost cotangent sums (thread 0 / thread of cell N-1)
    int bad_step = -1, bad_cell = 0;     // first non-finite cotangent this thread meets (the reverse sweep's first = the latest step)
    for (int step = T - 1; step >= 0; --step) {
        const float4 *tp = tape + ((size_t)step * L + lane) * tape_row;
        const float *gh = g_hist ? g_hist + ((size_t)step * L + lane) * 2 * N : nullptr;
        for (int k = t; k < N; k += B) {
            const float4 d0 = tp[k], d1 = tp[Np + k], d2 = tp[2 * Np + k];
            float gr = Gr[k + 1], gy = Gy[k + 1];
            if (gh) { gr += gh[k]; gy += gh[N + k]; }
            const float c0r = dot2(d0.x, gr, d0.z, gy), c0y = dot2(d0.y, gr, d0.w, gy);
            const float c1r = dot2(d1.x, gr, d1.z, gy), c1y = dot2(d1.y, gr, d1.w, gy);
            const float c2r = dot2(d2.x, gr, d2.z, gy), c2y = dot2(d2.y, gr, d2.w, gy);
            // c0 of cell k goes to cell k-1 (slot k), c2 of cell k goes to cell k+1 (slot k+2)
            C0r[k] = c0r; C0y[k] = c0y;
            C2r[k + 2] = c2r; C2y[k + 2] = c2y;
            Gr[k + 1] = c1r; Gy[k + 1] = c1y;
            if (k == 0) { ghl_r += (double)c0r; ghl_y += (double)c0y; }
            if (k == N - 1) { ghr_r += (double)c2r; ghr_y += (double)c2y; }
        }
        __syncthreads();
        for (int k = t; k < N; k += B) {
            // slot k+1 of C2 = c2 of cell k-1 (0 for k = 0); slot k+1 of C0 = c0 of cell k+1 (0 for k = N-1)
            const float c2lr = (k > 0) ? C2r[k + 1] : 0.f, c2ly = (k > 0) ? C2y[k + 1] : 0.f;
            const float c0rr = (k < N - 1) ? C0r[k + 1] : 0.f, c0ry = (k < N - 1) ? C0y[k + 1] : 0.f;
            const float nr = (Gr[k + 1] + c2lr) + c0rr;
            const float ny = (Gy[k + 1] + c2ly) + c0ry;
            Gr[k + 1] = nr; Gy[k + 1] = ny;
            if (bad_step < 0 && !(isfinite(nr) && isfinite(ny))) { bad_step = step; bad_cell = k; }
        }
        __syncthreads();
    }
    for (int k = t; k < N; k += B) { g_r_out[base + k] = Gr[k + 1]; g_y_out[base + k] = Gy[k + 1]; }
    if (g_ghost) {
        if (t == 0) { g_ghost[(size_t)lane * 4 + 0] = ghl_r; g_ghost[(size_t)lane * 4 + 1] = ghl_y; }
        if (t == (N - 1) % B) { g_ghost[(size_t)lane * 4 + 2] = ghr_r; g_ghost[(size_t)lane * 4 + 3] = ghr_y; }
    }
    if (bad_step >= 0) raise_fault(err, DHTS_FAULT_NAN, bad_step, lane, bad_cell);
}

// (A_i, B_i) of interface i from a tape row; SLOT[i] = the exception slot of interface i or 0xffff for a trivial one
// (tape_fill_slots: cleared, then filled from the row's idx list; the caller puts a barrier behind each of the two passes)
__device__ __forceinline__ void tape_iface(const float4 *row, const TapeGeom &geo, int N, int i,
                                           const unsigned short *SLOT, float4 &A, float4 &B) {
    const unsigned s = SLOT[i];
    if (s != 0xffffu) {
        const float4 *E = row + geo.s_f4 + geo.h_f4;
        A = E[2 * s]; B = E[2 * s + 1];
    } else {
        A = tape_trivial_A(reinterpret_cast<const TapeFp *>(row)[i < N ? i : N - 1]);
        B = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void tape_clear_slots(int N, unsigned short *SLOT, int t, int B) {
    for (int i = t; i <= N; i += B) SLOT[i] = 0xffffu;
}
__device__ __forceinline__ void tape_fill_slots(const float4 *row, const TapeGeom &geo, int N, unsigned short *SLOT, int t, int B) {
    const unsigned *H = tape_hdr(row, geo);
    const unsigned short *I = tape_idx(H, geo);
    int cnt = (int)H[0];
    if (cnt > N + 1) cnt = N + 1;
    for (int j = t; j < cnt; j += B) {
        const int i = I[j];
        if (i <= N) SLOT[i] = (unsigned short)j;
    }
}

// Reverse sweep over the rollout tape, one cell per thread (2 <= N <= blockDim.x <= 1024: the rollouts' common shape).  grid = L workgroups of `blockDim.x` threads (multiple of 64).
// Thread k owns cell k, whose blocks are made of the products of interfaces k and k + 1.  Where those are trivial it has them
// in registers (three floats each, read from the row's S block); thread j < cnt also carries exception j to its interface:
// (A, B) into XA / XB [interface], the step's tag into STAMP [interface], one barrier interval before they are used -- a cell
// whose interface carries the step's tag reads the products from there.  The cotangent of the own cell lives in a register;
// what the neighbours contribute goes through C0 / C2.  XA / XB / STAMP / C0 / C2 alternate between two copies with the step
// parity, so a step needs ONE barrier (LDS only: the tape loads stay in flight across it).  The tape entries are loaded
// three steps before they are needed (three register sets trading places, no moves), the exception counts six.
// WITHOUT per-step cotangents (kHist = kTaps = false) the trivial products take another road: every S entry is loaded once, by the
// thread of its interface, the right interface's entry comes from lane t + 1 by DPP moves (lane 63: from SB in LDS), and six S sets
// rotate through a six-step round (six = 2 LDS copies x 3 exception sets); the exceptions stay three sets deep.  Loads return in order: a wait for
// an exception set also waits for every S set issued before it, so FOUR S sets are in flight, two hold data that has arrived.
// The float32 arithmetic is that of the general kernel below
// (cell_blocks, dot2) two components at a time (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32: same operations, same roundings).
// Dynamic LDS: float2 C0[2][N + 2], C2[2][N + 2] (index k + 1 = cell k; slot 1 of C2 and slot N of C0 are never written and
// stay zero: the edge cells add 0) | float4 XA[2][N + 1], XB[2][N + 1] | u32 STAMP[2][N + 2] | without per-step cotangents:
// SEntry SB[2][kB / 64 + 1].
typedef float v2f __attribute__((ext_vector_type(2)));
struct alignas(16) SEntry { unsigned x, y, z; };      // an S entry in LDS: one 12-byte access at a 16-byte stride
__device__ __forceinline__ TapeFp tape_fp_bits(bits3 b) { TapeFp f; f.f0 = __uint_as_float(b.x); f.f2 = __uint_as_float(b.y); f.f3 = __uint_as_float(b.z); return f; }
__device__ __forceinline__ float4 f4_bits(bits4 b) { return make_float4(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)); }
__device__ __forceinline__ v2f pk_dot(v2f dlo, v2f dhi, v2f g) {           // (dot2(dlo.x, g.x, dhi.x, g.y), dot2(dlo.y, g.x, dhi.y, g.y))
    const v2f gx = {g.x, g.x}, gy = {g.y, g.y};
    return __builtin_elementwise_fma(dhi, gy, dlo * gx);
}
// (the planes are sized by the block, kB = 64 .. 512 threads >= N, so that every LDS address is a register plus a literal)
// deep: the instantiations without per-step cotangents add SEntry SB[2][kB / 64 + 1] (16 bytes each), the hand-over of the S entries
// at the wavefront boundaries
__host__ __device__ inline size_t bwd_fast_lds_bytes(int kB, bool deep) {
    return 2 * 2 * 8 * (size_t)(kB + 2) + 2 * 2 * 16 * (size_t)(kB + 2) + 2 * 4 * (size_t)(kB + 2) + (deep ? 2 * 16 * (size_t)(kB / 64 + 1) : 0);
}
// kHist: per-step cotangents g_hist [T][L][2][N] (a loss on the state history) are added to the cell's cotangent in front of
// every step; they ride in the register sets of the trivial products, three steps ahead.
// kFull: N = kB, every thread holds a cell (BASELINE config 2: 512 cells): no validity masks around the step's pieces.
// kSched: `g_ghost` is [T][L][2][2] (dhts_macro_rollout_bwd_sched): the two threads that sum the boundary cotangents store each step's
// addend instead, one 16-byte store per side and step.
// kTaps: `g_hist` is g_taps [T][L][2][n_det] (dhts_macro_rollout_bwd_taps), the cotangent of (r, y) of the cells det[j] after every step.
// It rides where the history's cotangent rides (same register sets, three steps ahead, the same g += gh_cur), but only a thread whose cell
// is a detector loads it -- from column dslot, its cell's place in det[] -- and everyone else holds zero: the sums are those of a dense
// g_hist that is zero elsewhere.  dslot comes out of an LDS map filled once (borrowed from C0 before the planes are zeroed): entry j of
// det[] is compared against [0, N) before it indexes the map, so an entry outside matches no cell, and dslot is -1 or a j < n_det.
template <int kB, bool kHist, bool kFull = false, bool kSched = false, bool kTaps = false>
__global__ __launch_bounds__(kB) __attribute__((amdgpu_waves_per_eu(4, 4))) void macro_rollout_bwd_fast_kernel(     // <= 128 VGPRs
    int L, int N, int T, double cc, const float4 *__restrict__ tape,
    const float *__restrict__ g_r_in, const float *__restrict__ g_y_in, const float *__restrict__ g_hist,
    float *__restrict__ g_r_out, float *__restrict__ g_y_out, double *__restrict__ g_ghost, dhts_error *err,
    const int32_t *__restrict__ det, int n_det) {
    static_assert(!(kHist && kTaps), "per-step cotangents come densely or at detectors, not both");
    constexpr bool kCot = kHist || kTaps;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    constexpr int B = kB;
    constexpr int P = kB + 2;
    float4 *XA = reinterpret_cast<float4 *>(lds), *XB = XA + 2 * P;                   // [copy][P]
    v2f *C0 = reinterpret_cast<v2f *>(XB + 2 * P), *C2 = C0 + 2 * P;                  // [copy][P]
    unsigned *STAMP = reinterpret_cast<unsigned *>(C2 + 2 * P);                       // [copy][P]
    SEntry *SB = reinterpret_cast<SEntry *>(STAMP + 2 * P);                           // [copy][kB / 64 + 1], !kCot only (104 P bytes in: 16-byte aligned)
    const size_t base = (size_t)lane * N;
    const TapeGeom geo = tape_geom(N);
    const v2f cf = {(float)cc, (float)cc}, ncf = {(float)(-cc), (float)(-cc)};
    const v2f zero2 = {0.f, 0.f}, e0 = {1.f, 0.f}, e1 = {0.f, 1.f};
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int k = t;
    const bool vk = kFull || k < N;
    const unsigned kl = vk ? k : N - 1;
    const unsigned kr = (kl + 1 < (unsigned)N) ? kl + 1 : N - 1;      // interface N is always an exception: its S entry does not exist
    // the wavefronts that hold cell 0 / cell N - 1 sum the ghosts' cotangents (a scalar: the test costs the others one s_cbranch)
    const int edge_wave = __builtin_amdgcn_readfirstlane(((t >> 6) == 0 || (t >> 6) == ((N - 1) >> 6)) ? 1 : 0);

    int dslot = -1;                      // kTaps: the column of this thread's cell in g_taps, -1 = not a detector
    if constexpr (kTaps) {
        int *MAP = reinterpret_cast<int *>(C0);          // [P] ints of the 4 P the two copies of C0 hold
        for (int i = t; i < P; i += B) MAP[i] = -1;
        __syncthreads();
        for (int j = t; j < n_det; j += B) {
            const unsigned dc = (unsigned)det[j];
            if (dc < (unsigned)N) MAP[dc] = j;
        }
        __syncthreads();
        if (vk) dslot = MAP[k];
        __syncthreads();
    }
    for (int i = t; i < 2 * P; i += B) { C0[i] = zero2; C2[i] = zero2; STAMP[i] = 0u; }
    if constexpr (!kCot) { if (t < 2 * (kB / 64 + 1)) SB[t] = SEntry{0u, 0u, 0u}; }
    v2f g = zero2;
    if (vk) g = v2f{g_r_in[base + k], g_y_in[base + k]};

    double gh_r = 0., gh_y = 0.;         // ghost cotangent sums: thread 0 the left ghost's, thread N - 1 the right one's
    // kSched: the row of the step, stepped down in front of every interval; slot 0 the left boundary's, slot 1 the right one's
    double2 *gs_run = kSched ? reinterpret_cast<double2 *>(g_ghost) + ((size_t)T * L + lane) * 2 : nullptr;
    int n_fin = 0;                       // checks of the cell's cotangent that found it finite: a non-finite one stays so (every later value is a
                                         // sum of products with it), so the count says where the first one appeared -- T + 1 checks, newest step first
    // byte offsets inside a row (32-bit, on top of the row's uniform base address)
    const unsigned off_sl = 12u * kl, off_sr = 12u * kr;
    const unsigned off_c = 16u * geo.s_f4;
    const unsigned off_i = 16u * geo.s_f4 + 8u + 2u * t;
    const unsigned off_e = 16u * (geo.s_f4 + geo.h_f4) + 32u * t;
    const size_t row_bytes = 16 * geo.row_f4;
    const char *tb = reinterpret_cast<const char *>(tape) + (size_t)lane * row_bytes;
    const size_t stride = (size_t)L * row_bytes;
    // (plain variables and macros, not structs handed to lambdas: those end up in scratch memory)
    // The two LDS copies are told apart by Q = (T - 1 - step) & 1; the three tape rows a step reads from are running pointers
    // (no multiplications in the loop).
    // per-step cotangents: row of step - 4 as well (the set refilled in the interval of `step` serves step - 4's blocks AND the
    // cotangent added in front of step - 4)
    const size_t hstride = (size_t)L * 2 * (kTaps ? n_det : N);
    const float *hb = kHist ? g_hist + (size_t)lane * 2 * N + kl : (kTaps ? g_hist + (size_t)lane * 2 * n_det : nullptr);
    const float *pH = kCot ? hb + (size_t)(T > 5 ? T - 5 : 0) * hstride : nullptr;
    const char *pS = tb + (size_t)(kCot ? (T > 5 ? T - 5 : 0) : (T > 8 ? T - 8 : 0)) * stride;      // row of step - 4 in the interval of `step` (!kCot: of step - 7)
    const char *pE = tb + (size_t)(T > 6 ? T - 6 : 0) * stride;      // row of step - 5
    const char *pC = tb + (size_t)(T > 9 ? T - 9 : 0) * stride;      // row of step - 8
#define DHTS_ROW(step_) (tb + (size_t)((step_) > 0 ? (step_) : 0) * stride)
    // Tape reads are BUFFER loads (round 5): the row's address is a scalar (the running pointer as the descriptor's base), the
    // thread's place in the row a 32-bit register -- no 64-bit vector add per load (the compiler forms one for a global load whose
    // zero-extended offset was hoisted out of the loop: six v_lshl_add_u64 per step), and always the vector memory path (vmcnt).
    const int row_rec = (int)row_bytes;
#define DHTS_RSRC(rb_) __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(rb_), 0, row_rec, 0x00020000)
#define DHTS_LOAD_CNT(rb_, c_) c_ = __builtin_amdgcn_raw_buffer_load_b32(DHTS_RSRC(rb_), off_c, 0, 0);
#define DHTS_LOAD_S(rb_, hp_, sl_, sr_, gh_)                                             \
    {                                                                                    \
        const __amdgpu_buffer_rsrc_t rs_ = DHTS_RSRC(rb_);                               \
        sl_ = tape_fp_bits(__builtin_amdgcn_raw_buffer_load_b96(rs_, off_sl, 0, 0));     \
        sr_ = tape_fp_bits(__builtin_amdgcn_raw_buffer_load_b96(rs_, off_sr, 0, 0));     \
        if (kHist) gh_ = v2f{(hp_)[0], (hp_)[N]};                                        \
        if (kTaps) { if (dslot >= 0) gh_ = v2f{(hp_)[dslot], (hp_)[n_det + dslot]}; }    \
    }
#define DHTS_LOAD_E(rb_, c_, ea_, eb_, ix_)                                              \
    if (t < (c_)) {                                                                      \
        const __amdgpu_buffer_rsrc_t rs_ = DHTS_RSRC(rb_);                               \
        ix_ = __builtin_amdgcn_raw_buffer_load_b16(rs_, off_i, 0, 0);                    \
        ea_ = f4_bits(__builtin_amdgcn_raw_buffer_load_b128(rs_, off_e, 0, 0));          \
        eb_ = f4_bits(__builtin_amdgcn_raw_buffer_load_b128(rs_, off_e + 16u, 0, 0));    \
    }
    // exception j of step_ to its interface, in LDS copy Q
#define DHTS_SCATTER(step_, Q, c_, ea_, eb_, ix_)                                        \
    {                                                                                    \
        if ((t < (c_)) & (ix_ <= (unsigned)N)) {                                         \
            XA[(Q) * P + ix_] = ea_; XB[(Q) * P + ix_] = eb_; STAMP[(Q) * P + ix_] = (unsigned)(step_) + 1u; \
        }                                                                                \
        if ((c_) > B) scatter_rest(step_, c_, XA + (Q) * P, XB + (Q) * P, STAMP + (Q) * P); \
    }
    // more exceptions than threads (the one-phase forward kernel flags every interface): the rest, without prefetch
    auto scatter_rest = [&](int step, int cnt, float4 *xa, float4 *xb, unsigned *st) {
        const float4 *row = reinterpret_cast<const float4 *>(DHTS_ROW(step));
        const unsigned short *I = tape_idx(tape_hdr(row, geo), geo);
        const float4 *E = row + geo.s_f4 + geo.h_f4;
        if (cnt > N + 1) cnt = N + 1;
        for (int j = t + B; j < cnt; j += B) {
            const int i = I[j];
            if (i <= N) { xa[i] = E[2 * j]; xb[i] = E[2 * j + 1]; st[i] = (unsigned)step + 1u; }
        }
    };
    // The blocks of step s_ from its products: the trivial ones in (sl_, sr_), the others in LDS copy Q (both stamps are read
    // before either product)
#define DHTS_BLOCKS(s_, Q, sl_, sr_)                                                     \
    {                                                                                    \
        const unsigned tag_ = (unsigned)(s_) + 1u;                                       \
        const unsigned st0_ = STAMP[(Q) * P + k], st1_ = STAMP[(Q) * P + k + 1];         \
        float4 aL = tape_trivial_A(sl_), bL = zero4, aR = tape_trivial_A(sr_), bR = zero4; \
        if (st0_ == tag_) { aL = XA[(Q) * P + k]; bL = XB[(Q) * P + k]; }                \
        if (st1_ == tag_) { aR = XA[(Q) * P + k + 1]; bR = XB[(Q) * P + k + 1]; }        \
        d0lo = ncf * -v2f{aL.x, aL.y}; d0hi = ncf * -v2f{aL.z, aL.w};                    \
        d2lo = ncf * v2f{bR.x, bR.y}; d2hi = ncf * v2f{bR.z, bR.w};                      \
        d1lo = e0 - cf * (v2f{aR.x, aR.y} - v2f{bL.x, bL.y});                            \
        d1hi = e1 - cf * (v2f{aR.z, aR.w} - v2f{bL.z, bL.w});                            \
    }
    // One barrier interval, step s, LDS copy Q (the neighbouring steps use copy R = 1 - Q).  Behind the barrier only what
    // depends on the neighbours: the cell's cotangent after step s + 1 (its own part c1v plus what the two neighbours left in
    // C0 / C2), the three products with the blocks of step s -- formed in the previous interval -- and their hand-over.  Then,
    // off that chain: the blocks of step s - 1 (trivial products in (sl_, sr_), exceptions scattered one interval ago), the
    // exceptions of step s - 2 from (ea_ .. ec_) to LDS, and the refills: exceptions of step s - 5 (their count cq_ arrived three
    // intervals ago), the count of step s - 8, the trivial products of step s - 4.  Everything read from the tape is in flight
    // for three intervals.  (This describes DHTS_STEP, the three-set interval; DHTS_CELL is shared with DHTS_STEP6, which has its own comment.)
#define DHTS_CELL(Q, R)                                                                  \
            g = (c1v + C2[(R) * P + k + 1]) + C0[(R) * P + k + 1];                       \
            if (kCot) g += gh_cur;                 /* the cotangent of the state after step s, if the loss looks at it */ \
            n_fin += (isfinite(g.x) && isfinite(g.y)) ? 1 : 0;                           \
            const v2f c0 = pk_dot(d0lo, d0hi, g), c2v = pk_dot(d2lo, d2hi, g);           \
            c1v = pk_dot(d1lo, d1hi, g);                                                 \
            /* c0 of cell k goes to cell k-1 (slot k), c2 of cell k goes to cell k+1 (slot k+2) */ \
            C0[(Q) * P + k] = c0;                                                        \
            C2[(Q) * P + k + 2] = c2v;                                                   \
            if (edge_wave) {                      /* a scalar branch: two wavefronts of the workgroup take it */ \
                if (kSched) {                                                            \
                    if (k == 0) gs_run[0] = make_double2((double)c0.x, (double)c0.y);    \
                    if (k == N - 1) gs_run[1] = make_double2((double)c2v.x, (double)c2v.y); \
                } else {                                                                 \
                if (k == 0) { gh_r += (double)c0.x; gh_y += (double)c0.y; }              \
                if (k == N - 1) { gh_r += (double)c2v.x; gh_y += (double)c2v.y; }        \
                }                                                                        \
            }
#define DHTS_STEP(CL, s_, Q, R, sl_, sr_, gh_, ea_, eb_, ix_, ec_, cq_)                  \
    {                                                                                    \
        if (kSched) gs_run -= 2 * (size_t)L;                                             \
        if (vk) {                                                                        \
            DHTS_CELL(Q, R)                                                              \
            if (!(CL) || (s_) >= 1) DHTS_BLOCKS((s_) - 1, R, sl_, sr_)                   \
            if (kCot) gh_cur = gh_;                /* of step s - 1: the set is refilled below */ \
        }                                                                                \
        if (!(CL) || (s_) >= 2) DHTS_SCATTER((s_) - 2, Q, ec_, ea_, eb_, ix_);           \
        ec_ = cq_;                                                                       \
        DHTS_LOAD_E(pE, ec_, ea_, eb_, ix_);                                             \
        DHTS_LOAD_CNT(pC, cq_);                                                          \
        DHTS_LOAD_S(pS, pH, sl_, sr_, gh_);                                              \
        if (kCot) pH -= (!(CL) || (s_) > 4) ? hstride : 0;                               \
        pS -= (!(CL) || (s_) > 4) ? stride : 0;                                          \
        pE -= (!(CL) || (s_) > 5) ? stride : 0;                                          \
        pC -= (!(CL) || (s_) > 8) ? stride : 0;                                          \
        lds_only_barrier();                                                              \
    }
    // after step 0, whose copy is Q = (T - 1) & 1
#define DHTS_LAST                                                                        \
    if (vk) {                                                                            \
        const int oq = ((T - 1) & 1) * P;                                                \
        g = (c1v + C2[oq + k + 1]) + C0[oq + k + 1];                                     \
        n_fin += (isfinite(g.x) && isfinite(g.y)) ? 1 : 0;                               \
    }
    if constexpr (kCot) {
    // ---- with per-step cotangents: the trivial products of both interfaces and the cotangent ride in three sets (sl, sr, gh)
    // register set A serves the steps T - 1, T - 4, ..., set B the steps T - 2, T - 5, ..., set C the steps T - 3, T - 6, ...
    TapeFp slA, srA, slB, srB, slC, srC;
    float4 eaA = zero4, ebA = zero4, eaB = zero4, ebB = zero4, eaC = zero4, ebC = zero4;
    unsigned ixA = 0, ixB = 0, ixC = 0;
    int ecA, ecB, ecC, cqA, cqB, cqC;
    v2f d0lo = zero2, d0hi = zero2, d1lo = zero2, d1hi = zero2, d2lo = zero2, d2hi = zero2;
    v2f c1v = g;                                          // "after step T": the incoming cotangent; C0 / C2 are zero
    DHTS_LOAD_CNT(DHTS_ROW(T - 1), ecA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 2), ecB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 3), ecC);
    DHTS_LOAD_CNT(DHTS_ROW(T - 4), cqA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 5), cqB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 6), cqC);
    DHTS_LOAD_E(DHTS_ROW(T - 1), ecA, eaA, ebA, ixA);
    DHTS_LOAD_E(DHTS_ROW(T - 2), ecB, eaB, ebB, ixB);
    DHTS_LOAD_E(DHTS_ROW(T - 3), ecC, eaC, ebC, ixC);
#define DHTS_HROW(step_) (hb + (size_t)((step_) > 0 ? (step_) : 0) * hstride)
    v2f ghA = zero2, ghB = zero2, ghC = zero2, gh_cur = zero2;
    DHTS_LOAD_S(DHTS_ROW(T - 1), DHTS_HROW(T - 1), slA, srA, ghA);
    DHTS_LOAD_S(DHTS_ROW(T - 2), DHTS_HROW(T - 2), slB, srB, ghB);
    DHTS_LOAD_S(DHTS_ROW(T - 3), DHTS_HROW(T - 3), slC, srC, ghC);
    __syncthreads();                                     // the zeroed planes
    DHTS_SCATTER(T - 1, 0, ecA, eaA, ebA, ixA);
    if (T >= 2) DHTS_SCATTER(T - 2, 1, ecB, eaB, ebB, ixB);
    ecA = cqA;
    ecB = cqB;
    DHTS_LOAD_E(DHTS_ROW(T - 4), ecA, eaA, ebA, ixA);
    DHTS_LOAD_E(DHTS_ROW(T - 5), ecB, eaB, ebB, ixB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 7), cqA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 8), cqB);
    lds_only_barrier();
    if (vk) DHTS_BLOCKS(T - 1, 0, slA, srA)
    if (kCot) gh_cur = ghA;                              // of step T - 1
    DHTS_LOAD_S(DHTS_ROW(T - 4), DHTS_HROW(T - 4), slA, srA, ghA);
    lds_only_barrier();                                  // (the first interval scatters step T - 3 into the copy these blocks were read from)
#undef DHTS_HROW
    // on entry to the interval of a step s of class A: the blocks of s are in registers, the exceptions of s - 1 in LDS;
    // (slB, srB) = S(s - 1), set C holds E(s - 2) and cqC the count of s - 5; (slC, srC) = S(s - 2), set A holds E(s - 3) and
    // cqA the count of s - 6; (slA, srA) = S(s - 3), set B holds E(s - 4) and cqB the count of s - 7
    int step = T - 1, q = 0;
    // the main loop: every row a step prefetches from exists (step - 2 > 8), so the running pointers move without end-of-tape
    // clamps and the "is there a step s - 1 / s - 2" tests are literals (round 5: 7 scalar instructions per pointer and step less)
    for (; step >= 11; step -= 3) {
        DHTS_STEP(0, step, q, q ^ 1, slB, srB, ghB, eaC, ebC, ixC, ecC, cqC)
        DHTS_STEP(0, step - 1, q ^ 1, q, slC, srC, ghC, eaA, ebA, ixA, ecA, cqA)
        DHTS_STEP(0, step - 2, q, q ^ 1, slA, srA, ghA, eaB, ebB, ixB, ecB, cqB)
        q ^= 1;
    }
    for (; step >= 2; step -= 3) {
        DHTS_STEP(1, step, q, q ^ 1, slB, srB, ghB, eaC, ebC, ixC, ecC, cqC)
        DHTS_STEP(1, step - 1, q ^ 1, q, slC, srC, ghC, eaA, ebA, ixA, ecA, cqA)
        DHTS_STEP(1, step - 2, q, q ^ 1, slA, srA, ghA, eaB, ebB, ixB, ecB, cqB)
        q ^= 1;
    }
    if (step >= 0) DHTS_STEP(1, step, q, q ^ 1, slB, srB, ghB, eaC, ebC, ixC, ecC, cqC)
    if (step >= 1) DHTS_STEP(1, step - 1, q ^ 1, q, slC, srC, ghC, eaA, ebA, ixA, ecA, cqA)
    DHTS_LAST
    } else {
    // ---- without per-step cotangents: every S entry is loaded ONCE, by the thread of its interface; six S sets rotate, four are in flight.
    // The right interface's entry comes from lane t + 1 (three wave_shl:1 DPP moves); lane 63 takes interface 64 (w + 1)'s from
    // SB [copy][wave], where lane 0 of every wavefront leaves its entry one interval before it is used (copy Q, like the exceptions:
    // same barrier).  SB [..][kB / 64] is never written: interface kB is interface N or past it, an exception whose STAMP test
    // picks XA / XB, like every interface N (whose thread holds the clamped entry N - 1 instead).
    // A set is three registers as loaded; S(x) is loaded in the interval of x + 7, handed over in that of x + 2, used in that of
    // x + 1.  The exceptions stay three sets deep; a set's count is a vector register while it is in flight and a scalar once it has
    // arrived, so nothing loaded is copied while it is in flight and the loop needs no wait at its back edge.
    constexpr int kNW1 = kB / 64 + 1;
    const unsigned wv = (unsigned)t >> 6;
#define DHTS_LOAD_S1(rb_, s_) s_ = __builtin_amdgcn_raw_buffer_load_b96(DHTS_RSRC(rb_), off_sl, 0, 0);
#define DHTS_HAND(Q, s_) if ((t & 63) == 0) SB[(Q) * kNW1 + wv] = SEntry{s_.x, s_.y, s_.z};
#define DHTS_BLOCKS1(st_, Q, s_)                                                         \
    {                                                                                    \
        const SEntry cw_ = SB[(Q) * kNW1 + wv + 1];                                      \
        const bits3 r_ = {take_right(s_.x, cw_.x), take_right(s_.y, cw_.y), take_right(s_.z, cw_.z)}; \
        const TapeFp sl1_ = tape_fp_bits(s_), sr1_ = tape_fp_bits(r_);                   \
        DHTS_BLOCKS(st_, Q, sl1_, sr1_)                                                  \
    }
    // More exceptions than threads: the rest, without prefetch, through the row's buffer descriptor.  (scatter_rest's per-thread
    // 64-bit addresses are hoisted out of the step loop as running pointers, two per unrolled step: 24 registers in a six-step round.
    // Here the thread's place in the row is a 32-bit offset, formed from the thread's number where it is needed: the empty asm
    // keeps the compiler from forming it once in front of the step loop and holding it in registers.)
    auto scatter_rest1 = [&](int step, int cnt, float4 *xa, float4 *xb, unsigned *st) {
        const __amdgpu_buffer_rsrc_t rs = DHTS_RSRC(DHTS_ROW(step));
        if (cnt > N + 1) cnt = N + 1;
        int t0 = t;
        asm volatile("" : "+v"(t0));
        for (int j = t0 + B; j < cnt; j += B) {
            const unsigned i = __builtin_amdgcn_raw_buffer_load_b16(rs, off_c + 8u + 2u * (unsigned)j, 0, 0);
            if (i <= (unsigned)N) {
                const unsigned oe = 16u * (geo.s_f4 + geo.h_f4) + 32u * (unsigned)j;
                xa[i] = f4_bits(__builtin_amdgcn_raw_buffer_load_b128(rs, oe, 0, 0));
                xb[i] = f4_bits(__builtin_amdgcn_raw_buffer_load_b128(rs, oe + 16u, 0, 0));
                st[i] = (unsigned)step + 1u;
            }
        }
    };
#define DHTS_SCATTER1(step_, Q, c_, ea_, eb_, ix_)                                       \
    {                                                                                    \
        if ((t < (c_)) & (ix_ <= (unsigned)N)) {                                         \
            XA[(Q) * P + ix_] = ea_; XB[(Q) * P + ix_] = eb_; STAMP[(Q) * P + ix_] = (unsigned)(step_) + 1u; \
        }                                                                                \
        if ((c_) > B) scatter_rest1(step_, c_, XA + (Q) * P, XB + (Q) * P, STAMP + (Q) * P); \
    }
    // a row's count is the same in every thread: once it has arrived it moves to a scalar register
#define DHTS_ARRIVED(h_, v_) h_ = __builtin_amdgcn_readfirstlane(v_);
    // One interval of step s as above; sb_ = S(s - 1), refilled with S(s - 7); sh_ = S(s - 2); h_ the count of the exceptions held
    // in (ea_, eb_, ix_), of step s - 2 and then of step s - 5; v_ the count of step s - 5, then that of step s - 8 in flight.
#define DHTS_STEP6(CL, s_, Q, R, sb_, sh_, ea_, eb_, ix_, h_, v_)                        \
    {                                                                                    \
        if (kSched) gs_run -= 2 * (size_t)L;                                             \
        if (vk) {                                                                        \
            DHTS_CELL(Q, R)                                                              \
            if (!(CL) || (s_) >= 1) DHTS_BLOCKS1((s_) - 1, R, sb_)                       \
        }                                                                                \
        /* the blocks are formed HERE: without a branch behind them (the masked forms have one) the compiler puts off the products */ \
        /* with cc until they are used, behind the barrier, and holds the sixteen factors instead of the twelve blocks */ \
        if (kFull) asm volatile("" : "+v"(d0lo), "+v"(d0hi), "+v"(d1lo), "+v"(d1hi), "+v"(d2lo), "+v"(d2hi)); \
        if (!(CL) || (s_) >= 2) DHTS_SCATTER1((s_) - 2, Q, h_, ea_, eb_, ix_);            \
        DHTS_ARRIVED(h_, v_)                                                             \
        DHTS_LOAD_E(pE, h_, ea_, eb_, ix_);                                              \
        DHTS_LOAD_CNT(pC, v_);                                                           \
        DHTS_LOAD_S1(pS, sb_);                                                           \
        pS -= (!(CL) || (s_) > 7) ? stride : 0;                                          \
        pE -= (!(CL) || (s_) > 5) ? stride : 0;                                          \
        pC -= (!(CL) || (s_) > 8) ? stride : 0;                                          \
        DHTS_HAND(Q, sh_)                                                                \
        lds_only_barrier();                                                              \
    }
    // the six steps of a round: S sets (B, C) (C, D) (D, E) (E, F) (F, A) (A, B), exception sets C A B C A B, LDS copies 0 1 0 1 0 1
#define DHTS_ROUND6(CL, X)                                                               \
        DHTS_STEP6(CL, step, 0, 1, sB, sC, eaC, ebC, ixC, hC, vC)                        \
        X(1) DHTS_STEP6(CL, step - 1, 1, 0, sC, sD, eaA, ebA, ixA, hA, vA)               \
        X(2) DHTS_STEP6(CL, step - 2, 0, 1, sD, sE, eaB, ebB, ixB, hB, vB)               \
        X(3) DHTS_STEP6(CL, step - 3, 1, 0, sE, sF, eaC, ebC, ixC, hC, vC)               \
        X(4) DHTS_STEP6(CL, step - 4, 0, 1, sF, sA, eaA, ebA, ixA, hA, vA)               \
        X(5) DHTS_STEP6(CL, step - 5, 1, 0, sA, sB, eaB, ebB, ixB, hB, vB)
    bits3 sA, sB, sC, sD, sE, sF;                        // S set A serves the steps T - 1, T - 7, ..., set F the steps T - 6, T - 12, ...
    float4 eaA = zero4, ebA = zero4, eaB = zero4, ebB = zero4, eaC = zero4, ebC = zero4;      // exception sets as above
    unsigned short ixA = 0, ixB = 0, ixC = 0;            // 16 bits as loaded: widened where it is used, not behind the load (a wait)
    int hA, hB, hC, vA, vB, vC;
    v2f d0lo = zero2, d0hi = zero2, d1lo = zero2, d1hi = zero2, d2lo = zero2, d2hi = zero2;
    v2f c1v = g;                                          // "after step T": the incoming cotangent; C0 / C2 are zero
    const v2f gh_cur = zero2;                             // (DHTS_CELL names it; no per-step cotangent here)
    DHTS_LOAD_CNT(DHTS_ROW(T - 1), vA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 2), vB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 3), vC);
    DHTS_ARRIVED(hA, vA)
    DHTS_ARRIVED(hB, vB)
    DHTS_ARRIVED(hC, vC)
    DHTS_LOAD_CNT(DHTS_ROW(T - 4), vA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 5), vB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 6), vC);
    DHTS_LOAD_E(DHTS_ROW(T - 1), hA, eaA, ebA, ixA);
    DHTS_LOAD_E(DHTS_ROW(T - 2), hB, eaB, ebB, ixB);
    DHTS_LOAD_E(DHTS_ROW(T - 3), hC, eaC, ebC, ixC);
    DHTS_LOAD_S1(DHTS_ROW(T - 1), sA);
    DHTS_LOAD_S1(DHTS_ROW(T - 2), sB);
    DHTS_LOAD_S1(DHTS_ROW(T - 3), sC);
    DHTS_LOAD_S1(DHTS_ROW(T - 4), sD);
    DHTS_LOAD_S1(DHTS_ROW(T - 5), sE);
    DHTS_LOAD_S1(DHTS_ROW(T - 6), sF);
    __syncthreads();                                     // the zeroed planes
    DHTS_SCATTER1(T - 1, 0, hA, eaA, ebA, ixA);
    if (T >= 2) DHTS_SCATTER1(T - 2, 1, hB, eaB, ebB, ixB);
    DHTS_HAND(0, sA)
    DHTS_HAND(1, sB)
    DHTS_ARRIVED(hA, vA)
    DHTS_ARRIVED(hB, vB)
    DHTS_LOAD_E(DHTS_ROW(T - 4), hA, eaA, ebA, ixA);
    DHTS_LOAD_E(DHTS_ROW(T - 5), hB, eaB, ebB, ixB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 7), vA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 8), vB);
    lds_only_barrier();
    if (vk) DHTS_BLOCKS1(T - 1, 0, sA)
    DHTS_LOAD_S1(DHTS_ROW(T - 7), sA);
    lds_only_barrier();                                  // (the first interval scatters step T - 3 into the copy these blocks were read from)
    // on entry to a round at step s: the blocks of s are in registers, the exceptions of s - 1 and SB of S(s - 1) in LDS copy 1;
    // sB .. sF, sA = S(s - 1) .. S(s - 6); set C holds E(s - 2), hC of them, and vC is the count of s - 5; set A holds E(s - 3)
    // and vA the count of s - 6; set B holds E(s - 4) and vB the count of s - 7.
    // A round is an even number of steps, so the LDS copies are literals.
    int step = T - 1;
    // the main loop: every row a step prefetches from exists (step - 5 > 8), so the running pointers move without end-of-tape
    // clamps and the "is there a step s - 1 / s - 2" tests are literals
#define DHTS_NO_EXIT(i_)
#define DHTS_EXIT(i_) if (step < (i_)) break;
    // The first round stands in front of the loop: the compiler sizes every wait in the loop for the fewest loads that can be
    // behind the awaited one on any path to it, and on the path from the prologue those are few -- entered from a round, the loop
    // sees the same loads in flight on both paths, and its back edge carries no wait (the three-set code above drains every load
    // there: its sets are copied at the back edge).
    if (step >= 14) {
        DHTS_ROUND6(0, DHTS_NO_EXIT)
        step -= 6;
        for (; step >= 14; step -= 6) { DHTS_ROUND6(0, DHTS_NO_EXIT) }
    }
    for (; step >= 0; step -= 6) { DHTS_ROUND6(1, DHTS_EXIT) }
#undef DHTS_ARRIVED
#undef DHTS_NO_EXIT
#undef DHTS_EXIT
#undef DHTS_ROUND6
#undef DHTS_STEP6
#undef DHTS_BLOCKS1
#undef DHTS_HAND
#undef DHTS_LOAD_S1
#undef DHTS_SCATTER1
    DHTS_LAST
    }
#undef DHTS_LAST
#undef DHTS_BLOCKS
#undef DHTS_ROW
#undef DHTS_LOAD_CNT
#undef DHTS_RSRC
#undef DHTS_LOAD_S
#undef DHTS_LOAD_E
#undef DHTS_SCATTER
#undef DHTS_CELL
#undef DHTS_STEP
    if (vk) { g_r_out[base + k] = g.x; g_y_out[base + k] = g.y; }
    if (!kSched && g_ghost) {
        if (t == 0) { g_ghost[(size_t)lane * 4 + 0] = gh_r; g_ghost[(size_t)lane * 4 + 1] = gh_y; }
        if (t == N - 1) { g_ghost[(size_t)lane * 4 + 2] = gh_r; g_ghost[(size_t)lane * 4 + 3] = gh_y; }
    }
    if (vk && n_fin < T + 1) raise_fault(err, DHTS_FAULT_NAN, n_fin == 0 ? T - 1 : T - n_fin, lane, k);      // (check i >= 1 looks at the state after step T - i)
}

// The same sweep with TWO cells per thread (cells t and t + kB; kB + 1 < N <= 2 kB): what lanes of 1026 .. 2048 cells take
// (kB = 1024) instead of the general kernel below.  (Measured as a replacement of the one-cell kernel at 1024 lanes x 512 cells
// in round 2 -- four workgroups per CU, every lane resident at once -- it lost, 2.50 against 1.82 ms: the sweep is bound by
// instruction issue and a thread with two cells issues as many instructions per cell as two threads with one.)
// Differences to the kernel above: the exceptions' products stay in the order of their list (XA / XB [slot], slot < kB; a
// row with more exceptions than that leaves the rest in HBM, where the cell that needs one reads it), STAMP [interface] carries
// (step tag << 12 | slot); two register sets instead of three (tape entries two intervals in flight, counts two more), so
// the two LDS copies are literals of the two-step loop body.
// Dynamic LDS: float2 C0[2][P], C2[2][P] | u32 STAMP[2][P] | float4 XA[2][kB], XB[2][kB]      (P = 2 kB + 2)
__host__ __device__ inline size_t bwd_fast2_lds_bytes(int kB) {
    const size_t P = 2 * (size_t)kB + 2;
    return 2 * 2 * 8 * P + 2 * 4 * P + 2 * 2 * 16 * (size_t)kB;
}
template <int kB, bool kFull, bool kSched = false>          // kFull: N = 2 kB, both cells of every thread exist (one basic block per interval); kSched: as above
__global__ __launch_bounds__(kB) __attribute__((amdgpu_waves_per_eu(4, 4))) void macro_rollout_bwd_fast2_kernel(     // <= 128 VGPRs
    int L, int N, int T, double cc, const float4 *__restrict__ tape,
    const float *__restrict__ g_r_in, const float *__restrict__ g_y_in,
    float *__restrict__ g_r_out, float *__restrict__ g_y_out, double *__restrict__ g_ghost, dhts_error *err) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    constexpr int B = kB;
    constexpr int P = 2 * kB + 2;
    float4 *XA = reinterpret_cast<float4 *>(lds), *XB = XA + 2 * kB;                  // [copy][kB]
    v2f *C0 = reinterpret_cast<v2f *>(XB + 2 * kB), *C2 = C0 + 2 * P;                 // [copy][P]
    unsigned *STAMP = reinterpret_cast<unsigned *>(C2 + 2 * P);                       // [copy][P]
    const size_t base = (size_t)lane * N;
    const TapeGeom geo = tape_geom(N);
    const v2f cf = {(float)cc, (float)cc}, ncf = {(float)(-cc), (float)(-cc)};
    const v2f zero2 = {0.f, 0.f}, e0 = {1.f, 0.f}, e1 = {0.f, 1.f};
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int ka = t, kb = t + kB;
    const bool va = kFull || ka < N, vb = kFull || kb < N;
    const unsigned la = va ? ka : N - 1, lb = vb ? kb : N - 1;

    for (int i = t; i < 2 * P; i += B) { C0[i] = zero2; C2[i] = zero2; STAMP[i] = 0u; }
    v2f ga = zero2, gb = zero2;
    if (va) ga = v2f{g_r_in[base + ka], g_y_in[base + ka]};
    if (vb) gb = v2f{g_r_in[base + kb], g_y_in[base + kb]};

    double gh_r = 0., gh_y = 0.;         // ghost cotangent sums: the thread of cell 0 the left ghost's, the thread of cell N - 1 the
                                         // right one's (never the same thread: the launcher keeps N = kB + 1 away from this kernel)
    double2 *gs_run = kSched ? reinterpret_cast<double2 *>(g_ghost) + ((size_t)T * L + lane) * 2 : nullptr;      // (as in the one-cell kernel)
    int bad_step = -1;                   // (first non-finite cotangent: step << 1 | which of the two cells)
    unsigned zv;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zv));     // keeps the count loads on the vector memory path (vmcnt, not lgkmcnt)
    // (the entry right of cell N - 1 does not exist -- interface N is always an exception -- and is never used: its 12 bytes are
    // read from the row's padding / header)
    const unsigned off_la = 12u * la, off_lb = 12u * lb;
    const unsigned off_c = 16u * geo.s_f4 + zv;
    const unsigned off_i = 16u * geo.s_f4 + 8u + 2u * t;
    const unsigned e_base = 16u * (geo.s_f4 + geo.h_f4);
    const unsigned off_e = e_base + 32u * t;
    const size_t row_bytes = 16 * geo.row_f4;
    const char *tb = reinterpret_cast<const char *>(tape) + (size_t)lane * row_bytes;
    const size_t stride = (size_t)L * row_bytes;
    const char *pS = tb + (size_t)(T > 4 ? T - 4 : 0) * stride;      // row of step - 3 in the interval of `step`
    const char *pE = tb + (size_t)(T > 5 ? T - 5 : 0) * stride;      // row of step - 4
    const char *pC = tb + (size_t)(T > 7 ? T - 7 : 0) * stride;      // row of step - 6
#define DHTS_ROW(step_) (tb + (size_t)((step_) > 0 ? (step_) : 0) * stride)
#define DHTS_LOAD_CNT(rb_, c_) c_ = *reinterpret_cast<const int *>((rb_) + off_c);
#define DHTS_LOAD_S(rb_, S_)                                                             \
    {                                                                                    \
        S_##la = *reinterpret_cast<const TapeFp *>((rb_) + off_la);                      \
        S_##ra = *reinterpret_cast<const TapeFp *>((rb_) + off_la + 12);                 \
        S_##lb = *reinterpret_cast<const TapeFp *>((rb_) + off_lb);                      \
        S_##rb = *reinterpret_cast<const TapeFp *>((rb_) + off_lb + 12);                 \
    }
    // (ix_ = interface of exception t, 0xffff where the list is shorter; the list's length rides in its upper half)
#define DHTS_LOAD_E(rb_, c_, ea_, eb_, ix_)                                              \
    ix_ = 0xffffu | ((unsigned)(c_) << 16);                                              \
    if (t < (c_)) {                                                                      \
        ix_ = *reinterpret_cast<const unsigned short *>((rb_) + off_i) | ((unsigned)(c_) << 16); \
        ea_ = *reinterpret_cast<const float4 *>((rb_) + off_e);                          \
        eb_ = *reinterpret_cast<const float4 *>((rb_) + off_e + 16);                     \
    }
    // exception j = t of step_ into copy Q; its interface's stamp points to it.  Exceptions beyond the block size stay in HBM.
#define DHTS_SCATTER(step_, Q, ea_, eb_, ix_)                                            \
    {                                                                                    \
        const unsigned i_ = (ix_) & 0xffffu;                                             \
        if (i_ <= (unsigned)N) {                                                         \
            XA[(Q) * kB + t] = ea_; XB[(Q) * kB + t] = eb_;                              \
            STAMP[(Q) * P + i_] = (((unsigned)(step_) + 1u) << 12) | (unsigned)t;        \
        }                                                                                \
        if ((int)((ix_) >> 16) > B) stamp_rest(step_, (int)((ix_) >> 16), STAMP + (Q) * P); \
    }
    auto stamp_rest = [&](int step, int cnt, unsigned *st) {
        const float4 *row = reinterpret_cast<const float4 *>(DHTS_ROW(step));
        const unsigned short *I = tape_idx(tape_hdr(row, geo), geo);
        if (cnt > N + 1) cnt = N + 1;
        for (int j = t + B; j < cnt; j += B) {
            const int i = I[j];
            if (i <= N) st[i] = (((unsigned)step + 1u) << 12) | (unsigned)j;
        }
    };
    // the products of interface i_ of step s_: exception (slot in LDS copy Q, or beyond the block size: in HBM) or trivial (s3_)
#define DHTS_PRODUCTS(s_, Q, i_, s3_, A_, B_)                                            \
    {                                                                                    \
        const unsigned st_ = STAMP[(Q) * P + (i_)];                                      \
        A_ = tape_trivial_A(s3_); B_ = zero4;                                            \
        if ((st_ >> 12) == (unsigned)(s_) + 1u) {                                        \
            const unsigned j_ = st_ & 4095u;                                             \
            if (j_ < (unsigned)kB) { A_ = XA[(Q) * kB + j_]; B_ = XB[(Q) * kB + j_]; }   \
            else {                                                                       \
                const float4 *E_ = reinterpret_cast<const float4 *>(DHTS_ROW(s_) + e_base); \
                A_ = E_[2 * j_]; B_ = E_[2 * j_ + 1];                                    \
            }                                                                            \
        }                                                                                \
    }
    // the blocks of cell k_ (suffix X_ = a / b) at step s_
#define DHTS_BLOCKS(s_, Q, k_, sl_, sr_, X_)                                             \
    {                                                                                    \
        float4 aL, bL, aR, bR;                                                           \
        DHTS_PRODUCTS(s_, Q, k_, sl_, aL, bL)                                            \
        DHTS_PRODUCTS(s_, Q, (k_) + 1, sr_, aR, bR)                                      \
        d0lo##X_ = ncf * -v2f{aL.x, aL.y}; d0hi##X_ = ncf * -v2f{aL.z, aL.w};            \
        d2lo##X_ = ncf * v2f{bR.x, bR.y}; d2hi##X_ = ncf * v2f{bR.z, bR.w};              \
        d1lo##X_ = e0 - cf * (v2f{aR.x, aR.y} - v2f{bL.x, bL.y});                        \
        d1hi##X_ = e1 - cf * (v2f{aR.z, aR.w} - v2f{bL.z, bL.w});                        \
    }
    // behind the barrier: the cell's cotangent after step s + 1, its three products with the blocks of step s, their hand-over
#define DHTS_CELL(s_, Q, R, k_, X_)                                                      \
    {                                                                                    \
        g##X_ = (c1##X_ + C2[(R) * P + (k_) + 1]) + C0[(R) * P + (k_) + 1];              \
        if (bad_step < 0 && !(isfinite(g##X_.x) && isfinite(g##X_.y))) bad_step = ((((s_) + 1 < T) ? (s_) + 1 : T - 1) << 1) | ((k_) == kb); \
        const v2f c0 = pk_dot(d0lo##X_, d0hi##X_, g##X_), c2v = pk_dot(d2lo##X_, d2hi##X_, g##X_); \
        c1##X_ = pk_dot(d1lo##X_, d1hi##X_, g##X_);                                      \
        C0[(Q) * P + (k_)] = c0;                                                         \
        C2[(Q) * P + (k_) + 2] = c2v;                                                    \
        if (__builtin_amdgcn_ballot_w64(((k_) == 0) | ((k_) == N - 1))) {                \
            asm volatile("" ::: "memory");          /* a real branch: two wavefronts of the workgroup take it */ \
            if (kSched) {                                                                \
                if ((k_) == 0) gs_run[0] = make_double2((double)c0.x, (double)c0.y);     \
                if ((k_) == N - 1) gs_run[1] = make_double2((double)c2v.x, (double)c2v.y); \
            } else {                                                                     \
            if ((k_) == 0) { gh_r += (double)c0.x; gh_y += (double)c0.y; }               \
            if ((k_) == N - 1) { gh_r += (double)c2v.x; gh_y += (double)c2v.y; }         \
            }                                                                            \
        }                                                                                \
    }
    // One barrier interval, step s (LDS copy Q, its neighbours' copy R = 1 - Q): the two cells' chain parts, then the blocks of
    // step s - 1 from the trivial products in set S_ and the exceptions scattered one interval ago, the exceptions of step s - 2
    // from (ea_ .. ec_) to LDS, and the refills: exceptions of step s - 4 (count cq_), the count of step s - 6, the trivial
    // products of step s - 3.
#define DHTS_STEP(s_, Q, R, S_, ea_, eb_, ix_, cq_)                                      \
    {                                                                                    \
        if (kSched) gs_run -= 2 * (size_t)L;                                             \
        if (va) DHTS_CELL(s_, Q, R, ka, a)                                               \
        if (vb) DHTS_CELL(s_, Q, R, kb, b)                                               \
        if ((s_) >= 1) {                                                                 \
            if (va) DHTS_BLOCKS((s_) - 1, R, ka, S_##la, S_##ra, a)                      \
            if (vb) DHTS_BLOCKS((s_) - 1, R, kb, S_##lb, S_##rb, b)                      \
        }                                                                                \
        if ((s_) >= 2) DHTS_SCATTER((s_) - 2, Q, ea_, eb_, ix_);                         \
        DHTS_LOAD_E(pE, cq_, ea_, eb_, ix_);                                             \
        DHTS_LOAD_CNT(pC, cq_);                                                          \
        DHTS_LOAD_S(pS, S_);                                                             \
        pS -= ((s_) > 3) ? stride : 0;                                                   \
        pE -= ((s_) > 4) ? stride : 0;                                                   \
        pC -= ((s_) > 6) ? stride : 0;                                                   \
        lds_only_barrier();                                                              \
    }
    // register set A serves the steps T - 1, T - 3, ..., set B the steps T - 2, T - 4, ...
    TapeFp SAla, SAra, SAlb, SArb, SBla, SBra, SBlb, SBrb;
    float4 eaA = zero4, ebA = zero4, eaB = zero4, ebB = zero4;
    unsigned ixA = 0, ixB = 0;
    int cqA, cqB;
    v2f d0loa = zero2, d0hia = zero2, d1loa = zero2, d1hia = zero2, d2loa = zero2, d2hia = zero2;
    v2f d0lob = zero2, d0hib = zero2, d1lob = zero2, d1hib = zero2, d2lob = zero2, d2hib = zero2;
    v2f c1a = ga, c1b = gb;                               // "after step T": the incoming cotangent; C0 / C2 are zero
    DHTS_LOAD_CNT(DHTS_ROW(T - 1), cqA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 2), cqB);
    DHTS_LOAD_E(DHTS_ROW(T - 1), cqA, eaA, ebA, ixA);
    DHTS_LOAD_E(DHTS_ROW(T - 2), cqB, eaB, ebB, ixB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 3), cqA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 4), cqB);
    DHTS_LOAD_S(DHTS_ROW(T - 1), SA);
    DHTS_LOAD_S(DHTS_ROW(T - 2), SB);
    __syncthreads();                                     // the zeroed planes
    DHTS_SCATTER(T - 1, 0, eaA, ebA, ixA);
    if (T >= 2) DHTS_SCATTER(T - 2, 1, eaB, ebB, ixB);
    DHTS_LOAD_E(DHTS_ROW(T - 3), cqA, eaA, ebA, ixA);
    DHTS_LOAD_E(DHTS_ROW(T - 4), cqB, eaB, ebB, ixB);
    DHTS_LOAD_CNT(DHTS_ROW(T - 5), cqA);
    DHTS_LOAD_CNT(DHTS_ROW(T - 6), cqB);
    lds_only_barrier();
    if (va) DHTS_BLOCKS(T - 1, 0, ka, SAla, SAra, a)
    if (vb) DHTS_BLOCKS(T - 1, 0, kb, SAlb, SArb, b)
    DHTS_LOAD_S(DHTS_ROW(T - 3), SA);
    lds_only_barrier();                                  // (the first interval scatters step T - 3 into the copy these blocks were read from)
    // on entry to the interval of a step s of class A: the blocks of s are in registers, the exceptions of s - 1 in LDS copy 1;
    // set B holds S(s - 1) and E(s - 3), cqB the count of s - 5; set A holds S(s - 2) and E(s - 2), cqA the count of s - 4
    int step = T - 1;
    for (; step >= 1; step -= 2) {
        DHTS_STEP(step, 0, 1, SB, eaA, ebA, ixA, cqA)
        DHTS_STEP(step - 1, 1, 0, SA, eaB, ebB, ixB, cqB)
    }
    if (step == 0) DHTS_STEP(0, 0, 1, SB, eaA, ebA, ixA, cqA)
    {                                                    // after step 0, whose copy is (T - 1) & 1
        const int oq = ((T - 1) & 1) * P;
        if (va) { ga = (c1a + C2[oq + ka + 1]) + C0[oq + ka + 1]; if (bad_step < 0 && !(isfinite(ga.x) && isfinite(ga.y))) bad_step = 0; }
        if (vb) { gb = (c1b + C2[oq + kb + 1]) + C0[oq + kb + 1]; if (bad_step < 0 && !(isfinite(gb.x) && isfinite(gb.y))) bad_step = 1; }
    }
#undef DHTS_ROW
#undef DHTS_LOAD_CNT
#undef DHTS_LOAD_S
#undef DHTS_LOAD_E
#undef DHTS_SCATTER
#undef DHTS_PRODUCTS
#undef DHTS_BLOCKS
#undef DHTS_CELL
#undef DHTS_STEP
    if (va) { g_r_out[base + ka] = ga.x; g_y_out[base + ka] = ga.y; }
    if (vb) { g_r_out[base + kb] = gb.x; g_y_out[base + kb] = gb.y; }
    if (!kSched && g_ghost) {
        if (ka == 0) { g_ghost[(size_t)lane * 4 + 0] = gh_r; g_ghost[(size_t)lane * 4 + 1] = gh_y; }
        if (ka == N - 1 || kb == N - 1) { g_ghost[(size_t)lane * 4 + 2] = gh_r; g_ghost[(size_t)lane * 4 + 3] = gh_y; }
    }
    if (bad_step >= 0) raise_fault(err, DHTS_FAULT_NAN, bad_step >> 1, lane, (bad_step & 1) ? kb : ka);
}

// Reverse sweep over the rollout tape, any lane length (lanes above 1024 cells, single cells), per-step cotangents (g_hist) or not.
// grid = L workgroups of `blockDim.x` threads (multiple of 64).  Dynamic LDS: 6 planes of (N + 2) floats | u16 SLOT[N + 1].
// kSched: `g_ghost` is [T][L][2][2]: every step's boundary addend is stored instead of summed.
// kTaps: `g_hist` is g_taps [T][L][2][n_det]: in front of every step thread j adds column j to the cotangent of cell det[j] in LDS (an entry
// outside [0, N) is skipped before it forms an address), beside the slot clearing, two barriers ahead of the loop that reads the cells:
// the same float32 sum as gr += gh[k] with a dense g_hist.  What lanes of 1026 .. 2048 cells take with detectors, as with a history.
template <bool kSched = false, bool kTaps = false>
__global__ __launch_bounds__(512) void macro_rollout_bwd_kernel(
    int L, int N, int T, double cc, const float4 *__restrict__ tape,
    const float *__restrict__ g_r_in, const float *__restrict__ g_y_in, const float *__restrict__ g_hist,
    float *__restrict__ g_r_out, float *__restrict__ g_y_out, double *__restrict__ g_ghost, dhts_error *err,
    const int32_t *__restrict__ det, int n_det) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = blockIdx.x;
    const int t = threadIdx.x;
    const int B = blockDim.x;
    const int P = N + 2;
    const BwdPlanes pl = bwd_planes(lds, P);
    float *Gr = pl.Gr, *Gy = pl.Gy, *C0r = pl.C0r, *C0y = pl.C0y, *C2r = pl.C2r, *C2y = pl.C2y;
    float *xbase = lds + ((6 * P + 3) & ~3);
    const size_t base = (size_t)lane * N;
    const TapeGeom geo = tape_geom(N);
    const float cf = (float)cc, ncf = (float)(-cc);

    for (int k = t; k < P; k += B) { C0r[k] = 0.f; C0y[k] = 0.f; C2r[k] = 0.f; C2y[k] = 0.f; Gr[k] = 0.f; Gy[k] = 0.f; }
    __syncthreads();
    for (int k = t; k < N; k += B) { Gr[k + 1] = g_r_in[base + k]; Gy[k + 1] = g_y_in[base + k]; }
    __syncthreads();

    double ghl_r = 0., ghl_y = 0., ghr_r = 0., ghr_y = 0.;   // ghost cotangent sums (thread 0 / thread of cell N-1)
    int bad_step = -1, bad_cell = 0;     // first non-finite cotangent this thread meets (the reverse sweep's first = the latest step)
    {
        unsigned short *SLOT = reinterpret_cast<unsigned short *>(xbase);
        for (int step = T - 1; step >= 0; --step) {
            const float4 *row = tape + ((size_t)step * L + lane) * geo.row_f4;
            const float *gh = (!kTaps && g_hist) ? g_hist + ((size_t)step * L + lane) * 2 * N : nullptr;
            if constexpr (kTaps) {
                const float *gt = g_hist + ((size_t)step * L + lane) * 2 * n_det;
                for (int j = t; j < n_det; j += B) {
                    const unsigned dc = (unsigned)det[j];
                    if (dc < (unsigned)N) { Gr[dc + 1] += gt[j]; Gy[dc + 1] += gt[n_det + j]; }
                }
            }
            tape_clear_slots(N, SLOT, t, B);
            __syncthreads();
            tape_fill_slots(row, geo, N, SLOT, t, B);
            __syncthreads();
            for (int k = t; k < N; k += B) {
                float4 aL, bL, aR, bR, d0, d1, d2;
                tape_iface(row, geo, N, k, SLOT, aL, bL);
                tape_iface(row, geo, N, k + 1, SLOT, aR, bR);
                cell_blocks(aL, bL, aR, bR, cf, ncf, d0, d1, d2);
                float gr = Gr[k + 1], gy = Gy[k + 1];
                if (gh) { gr += gh[k]; gy += gh[N + k]; }
                const float c0r = dot2(d0.x, gr, d0.z, gy), c0y = dot2(d0.y, gr, d0.w, gy);
                const float c1r = dot2(d1.x, gr, d1.z, gy), c1y = dot2(d1.y, gr, d1.w, gy);
                const float c2r = dot2(d2.x, gr, d2.z, gy), c2y = dot2(d2.y, gr, d2.w, gy);
                C0r[k] = c0r; C0y[k] = c0y;
                C2r[k + 2] = c2r; C2y[k + 2] = c2y;
                Gr[k + 1] = c1r; Gy[k + 1] = c1y;
                if constexpr (kSched) {
                    double2 *gs = reinterpret_cast<double2 *>(g_ghost) + ((size_t)step * L + lane) * 2;
                    if (k == 0) gs[0] = make_double2((double)c0r, (double)c0y);
                    if (k == N - 1) gs[1] = make_double2((double)c2r, (double)c2y);
                } else {
                    if (k == 0) { ghl_r += (double)c0r; ghl_y += (double)c0y; }
                    if (k == N - 1) { ghr_r += (double)c2r; ghr_y += (double)c2y; }
                }
            }
            __syncthreads();
            for (int k = t; k < N; k += B) {
                const float c2lr = (k > 0) ? C2r[k + 1] : 0.f, c2ly = (k > 0) ? C2y[k + 1] : 0.f;
                const float c0rr = (k < N - 1) ? C0r[k + 1] : 0.f, c0ry = (k < N - 1) ? C0y[k + 1] : 0.f;
                const float nr = (Gr[k + 1] + c2lr) + c0rr;
                const float ny = (Gy[k + 1] + c2ly) + c0ry;
                Gr[k + 1] = nr; Gy[k + 1] = ny;
                if (bad_step < 0 && !(isfinite(nr) && isfinite(ny))) { bad_step = step; bad_cell = k; }
            }
            __syncthreads();
        }
    }
    for (int k = t; k < N; k += B) { g_r_out[base + k] = Gr[k + 1]; g_y_out[base + k] = Gy[k + 1]; }
    if (!kSched && g_ghost) {
        if (t == 0) { g_ghost[(size_t)lane * 4 + 0] = ghl_r; g_ghost[(size_t)lane * 4 + 1] = ghl_y; }
        if (t == (N - 1) % B) { g_ghost[(size_t)lane * 4 + 2] = ghr_r; g_ghost[(size_t)lane * 4 + 3] = ghr_y; }
    }
    if (bad_step >= 0) raise_fault(err, DHTS_FAULT_NAN, bad_step, lane, bad_cell);
}

// The reference's cell blocks dqs[a][3][2][2] of every (step, lane) from the rollout tape, in the single-step operator's
// layout [step][lane][3][Np][4], formed with the reverse sweep's own code.  grid = T * L workgroups; LDS = u16 SLOT[N + 1].
__global__ void macro_tape_expand_kernel(int N, double cc, const float4 *__restrict__ tape, float4 *__restrict__ dqs) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned short *SLOT = reinterpret_cast<unsigned short *>(lds);
    const TapeGeom geo = tape_geom(N);
    const int Np = (N + 63) & ~63;
    const float4 *row = tape + (size_t)blockIdx.x * geo.row_f4;
    float4 *out = dqs + (size_t)blockIdx.x * 3 * Np;
    const float cf = (float)cc, ncf = (float)(-cc);
    tape_clear_slots(N, SLOT, threadIdx.x, blockDim.x);
    __syncthreads();
    tape_fill_slots(row, geo, N, SLOT, threadIdx.x, blockDim.x);
    __syncthreads();
    for (int k = threadIdx.x; k < Np; k += blockDim.x) {
        float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f), d1 = d0, d2 = d0;      // the padding is written too (zeros)
        if (k < N) {
            float4 aL, bL, aR, bR;
            tape_iface(row, geo, N, k, SLOT, aL, bL);
            tape_iface(row, geo, N, k + 1, SLOT, aR, bR);
            cell_blocks(aL, bL, aR, bR, cf, ncf, d0, d1, d2);
        }
        out[k] = d0; out[Np + k] = d1; out[2 * Np + k] = d2;
    }
}

// ---- known-answer entry: n independent interfaces, both solver variants ---------------------------------
// in [9][n] double = rL yL uL ueqL rR yR uR ueqR u_max (SoA); variant 0 = production, 1 = reference-order IEEE
__global__ void arz_interface_batch_kernel(int64_t n, int variant, const double *__restrict__ in, double dt, double dx,
                                           int32_t *__restrict__ ci, double *__restrict__ q0, double *__restrict__ flux,
                                           float *__restrict__ dL, float *__restrict__ dR, float *__restrict__ fp,
                                           float *__restrict__ A, float *__restrict__ B, int32_t *__restrict__ cfl_bad,
                                           double *__restrict__ speed) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        IfaceConst kc;
        kc.set_um(in[8 * n + i]); kc.set_grid(dt, dx);
        Iface f;
        IfaceDebug dbg;
        if (variant == 1)
            arz_interface_ieee(in[i], in[n + i], in[2 * n + i], in[3 * n + i], in[4 * n + i], in[5 * n + i], in[6 * n + i],
                               in[7 * n + i], kc, f, &dbg);
        else
            arz_interface_fast(in[i], in[n + i], in[2 * n + i], in[3 * n + i], in[4 * n + i], in[5 * n + i], in[6 * n + i],
                               in[7 * n + i], kc, f, &dbg);
        ci[i] = dbg.ci;
        flux[i] = f.Fr; flux[n + i] = f.Fy;
        cfl_bad[i] = f.cfl_bad ? 1 : 0;
        if (speed) { speed[i] = dbg.speed[0]; speed[n + i] = dbg.speed[1]; }
        for (int j = 0; j < 4; ++j) {
            q0[j * n + i] = dbg.q0[j];
            dL[j * n + i] = dbg.dL[j]; dR[j * n + i] = dbg.dR[j]; fp[j * n + i] = dbg.fp[j];
            A[j * n + i] = f.A[j]; B[j * n + i] = f.B[j];
        }
    }
}

// ---- elementwise float32 glue ------------------------------------------------------------------------
__global__ void macro_state_from_ru_kernel(int64_t n, float um, const float *__restrict__ r, const float *__restrict__ u,
                                           float *__restrict__ y, float *__restrict__ q) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float yy, qq;
        glue_from_r_u(r[i], u[i], um, yy, qq);
        y[i] = yy;
        q[i] = qq;
    }
}
__global__ void macro_state_from_ru_bwd_kernel(int64_t n, float um, const float *__restrict__ r, const float *__restrict__ u,
                                               const float *__restrict__ g_y, float *__restrict__ g_r, float *__restrict__ g_u) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gr = g_r[i], gu = 0.f;
        glue_y_bwd(r[i], u[i], um, g_y[i], gr, gu);
        g_r[i] = gr;
        g_u[i] = gu;
    }
}
__global__ void macro_u_tap_bwd_kernel(int64_t n, float um, const float *__restrict__ r, const float *__restrict__ y,
                                       const float *__restrict__ g_u, float *__restrict__ g_r, float *__restrict__ g_y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gr = g_r[i], gy = g_y[i];
        glue_u_bwd(r[i], y[i], um, g_u[i], gr, gy);
        g_r[i] = gr;
        g_y[i] = gy;
    }
}

// ---- forward-mode tangent sweep over the rollout tape (dhts_macro_rollout_jvp) and its glue ----------------------
#include "macro_jvp.inc"

// How a lane of the tape-free kernels (macro_fwd_jvp.inc, macro_ckpt.inc) ends: in two boundary cells that are data -- constant, or a
// schedule [T][L][2][4], what `bool kSched` says in the taped kernels above -- or in itself, a ring.
enum MacroBoundary { kBoundConst = 0, kBoundSched = 1, kBoundRing = 2 };

// ---- the rollout and its tangents in one kernel, no tape (dhts_macro_rollout_fwd_jvp) ----------------------------
#include "macro_fwd_jvp.inc"

// ---- reverse mode from checkpoints, the segment's interface products in LDS (dhts_macro_rollout_fwd_ckpt / _bwd_ckpt) ----
#define DHTS_MACRO_TARGET 0
#include "macro_ckpt.inc"
#undef DHTS_MACRO_TARGET
// ---- the dense-fit loss inside the checkpointed pair (dhts_macro_rollout_*_ckpt_target): the text of macro_ckpt.inc once more ----
#define DHTS_MACRO_TARGET 1
#include "macro_ckpt.inc"
#undef DHTS_MACRO_TARGET

}  // namespace dhts

// ---- C ABI -----------------------------------------------------------------------------------------------
using namespace dhts;

static inline bool macro_desc_ok(const dhts_macro_desc *d) {
    return d && d->n_lanes > 0 && d->n_cells > 0 && d->n_cells <= DHTS_MACRO_MAX_CELLS && d->dt > 0 && d->dx > 0 && d->u_max > 0;
}
// test / tuning hooks (dhts_set_option, dhts_common.hip): force the number of wavefronts per lane of the forward kernel (0 = heuristic);
// select the rollout forward kernel (0 = two-phase kernels, 1 = the one-phase kernel the single-step operator uses, 2 = no pair kernel)
int dhts_fwd_waves_override = 0;
int dhts_fwd_variant = 0;
int dhts_fwd_rotate = 1;        // DHTS_OPT_MACRO_FWD_ROTATE: priority rotation between the two halves of the pair kernel's grid
int dhts_fwd_group = 0;         // DHTS_OPT_MACRO_FWD_GROUP: traffic lanes per workgroup in the two-phase forward kernel (0 = heuristic)
int dhts_jvp_variant = 0;       // DHTS_OPT_MACRO_JVP_VARIANT: 1 = the general tangent sweep for every shape

static inline size_t fwd2_lds_bytes(int N) {
    return sizeof(CellRec) * (size_t)(N + 2) + 16 * (size_t)(N + 1) + sizeof(int) * (size_t)(N + 2) + 16;
}
// The pair kernel (macro_fwd_pairs.inc) takes full lanes of 128 W cells without a state history; traffic lanes per workgroup as
// for the lane-group kernel (four up to three wavefronts per lane, else two; one where the launch would leave CUs without a
// workgroup or the lanes do not divide).  0 = not this kernel (DHTS_OPT_MACRO_FWD_VARIANT = 2 turns it off).
static inline int macro_fwd3_group(const dhts_macro_desc *d, bool want_hist) {
    if (dhts_fwd_variant != 0 || want_hist || d->n_cells < 128 || d->n_cells % 128 != 0 || d->n_cells > 1024) return 0;
    const int W = d->n_cells / 128;
    if (dhts_fwd_waves_override > 0 && dhts_fwd_waves_override != W) return 0;       // (a forced wave count means the lane kernel)
    // lanes per workgroup: four for lanes of up to three wavefronts, one for four (1024 x 512: 2.59 against 2.65 ms for two,
    // 512 x 512: 0.93 / 1.10), two above (profiles/r04k_*, r04q_*)
    int G = dhts_fwd_group > 0 ? dhts_fwd_group : (W <= 3 ? 4 : (W == 4 ? 1 : 2));
    while (G > 1 && (d->n_lanes % G != 0 || (dhts_fwd_group == 0 && d->n_lanes / G < 256) || 64 * W * G > 1024 ||
                     (size_t)G * fwd3_region_bytes(d->n_cells) > 160 * 1024))
        G >>= 1;
    if ((size_t)G * fwd3_region_bytes(d->n_cells) > 160 * 1024) return 0;
    return G;
}

// The lane mapping of the two-phase lane kernel, which the fused forward + tangent kernel and the checkpointed pair share: W wavefronts
// per lane, each of p 64-cell passes -- of the W0 a caller asks for at most `cap`, then the fewest wavefronts that cover the lane with
// that many passes.  W0 (with or without DHTS_OPT_MACRO_FWD_WAVES) and the cap are the caller's.
struct MacroLaneMap { int W, p; };
static MacroLaneMap macro_lane_map(int N, int W0, int cap) {
    const int W = W0 > cap ? cap : (W0 < 1 ? 1 : W0);
    const int p = (N + 64 * W - 1) / (64 * W);
    return {(N + 64 * p - 1) / (64 * p), p};
}

// Which kernel instantiations dhts_macro_rollout_fwd / _bwd launch for a shape, decided here once: the launches switch on these fields
// and dhts_macro_rollout_plan copies them out.
enum { kMacroFwdLane = 0, kMacroFwdOnePhase = 1, kMacroFwdPair = 2 };      // plan[0]
enum { kMacroBwdGeneral = 0, kMacroBwdFast = 1, kMacroBwdFast2 = 2 };      // plan[4]
struct MacroPlan {
    bool hist, tape;      // what the caller asks for: the state history resp. per-step cotangents; the tape
    int fwd;              // forward kernel
    int W, p;             // two-phase kernels: wavefronts per lane, 64-cell passes per wavefront (0, 0: the one-phase kernel plans its own)
    bool dense;           // two-phase kernels: every thread-pass owns a cell, no history (kFull)
    int G;                // traffic lanes per workgroup (the pair kernel; 1 otherwise)
    size_t lds_fwd;       // two-phase kernels
    int bwd, bwd_block;   // reverse kernel and its threads per lane
    bool bwd_full;        // fast: N = block (128 .. 512, no dense per-step cotangents); fast2: N = 2 x block
    size_t lds_bwd;
};
// taps: the detector form (dhts_macro_rollout_fwd_taps / _bwd_taps): the plan of the same shape WITHOUT a history, except that lanes of
// 1026 .. 2048 cells take the general reverse sweep (the two-cells-per-thread kernel carries no per-step cotangents), as with a history
static MacroPlan macro_plan(const dhts_macro_desc *d, int T, bool want_hist, bool want_tape, bool taps = false) {
    MacroPlan pl = {};
    const int N = d->n_cells;
    pl.hist = want_hist; pl.tape = want_tape; pl.G = 1;
    // lanes whose records do not fit the two-phase kernels' LDS take the one-phase kernel (same tape format)
    if (dhts_fwd_variant == 1 || fwd2_lds_bytes(N) > 160 * 1024) {
        pl.fwd = kMacroFwdOnePhase;
    } else {
        // Wavefronts per lane of the two-phase forward kernel: two 64-cell passes per wavefront whenever the lane fits 16 of them -- the
        // two passes of a thread are independent instruction streams, and at 1024 x 512 the four-wave workgroups of all lanes are
        // resident at once (4 per CU) instead of taking two rounds.  Measured (tools/sweep_fwd_waves.py, forward ms for 1 / 2 / 4 / 8 /
        // 16 waves per lane; literal pass counts 1, 2, run-time above):
        //   1024 x 512: 7.5 / 3.95 / 3.50 / 4.07 / -      4096 x 256: 9.3 / 7.50 / 7.93 / - / -      256 x 2048: 19.6 / 10.7 / 6.0 / 4.09 / 3.54
        const MacroLaneMap m = macro_lane_map(N, dhts_fwd_waves_override > 0 ? dhts_fwd_waves_override : (N + 127) / 128, 16);
        pl.W = m.W; pl.p = m.p;
        pl.dense = (pl.p == 1 || pl.p == 2) && N == 64 * pl.p * pl.W && !want_hist;
        const int G = macro_fwd3_group(d, want_hist);
        pl.fwd = G > 0 ? kMacroFwdPair : kMacroFwdLane;
        if (G > 0) pl.G = G;
        pl.lds_fwd = G > 0 ? (size_t)G * fwd3_region_bytes(N) : fwd2_lds_bytes(N);
    }
    if (N >= 2 && N <= 1024 && T > 0) {       // (T = 0: no tape to prefetch from)
        pl.bwd = kMacroBwdFast;
        pl.bwd_block = N <= 64 ? 64 : (N <= 128 ? 128 : (N <= 256 ? 256 : (N <= 512 ? 512 : 1024)));
        pl.bwd_full = !want_hist && N == pl.bwd_block && N >= 128 && N <= 512;
        pl.lds_bwd = bwd_fast_lds_bytes(pl.bwd_block, !want_hist && !taps);
    } else if (N > 1025 && N <= 2048 && T > 0 && T < (1 << 20) - 1 && !want_hist && !taps) {
        // the two-cells-per-thread sweep (1024 threads): lanes of 1026 .. 2048 cells without per-step cotangents (the step tag has 20 bits)
        pl.bwd = kMacroBwdFast2;
        pl.bwd_block = 1024;
        pl.bwd_full = N == 2048;
        pl.lds_bwd = bwd_fast2_lds_bytes(1024);
    } else {
        pl.bwd = kMacroBwdGeneral;
        pl.bwd_block = padded64(N) > 512 ? 512 : padded64(N);
        pl.lds_bwd = sizeof(float) * (size_t)((6 * (N + 2) + 3) & ~3) + 2 * (size_t)(N + 1);
    }
    return pl;
}

// The form of a rollout call: what it takes besides the state, the boundary cells and the tape or the checkpoints.  Every rollout entry
// point -- taped, tangent, fused and checkpointed -- fills one and hands it to its launcher; kSched, kTaps and the target kernels are
// picked from it like every other template argument, so a further form is one more field here and one more pick there.
struct MacroForm {
    MacroBoundary bound;  // kBoundSched: the boundary cells are a schedule [T][L][2][4]; g_ghost is per step [T][L][2][2].  kBoundRing (the
                          // tape-free launchers only): no boundary cells -- `ghost`, g_ghost and the boundary tangents are NULL
    bool sched() const { return bound == kBoundSched; }
    const int32_t *det;   // detector cells [n_det], NULL: none
    int n_det;
    float *hist, *taps;   // forward: the state history [T][L][3][N] (not with detectors) resp. the readings [T][L][3][n_det]
    const float *g_cot;   // reverse: the per-step cotangents, g_hist [T][L][2][N] or with detectors g_taps [T][L][2][n_det]; NULL: none
    // the dense fit of the checkpointed pair: target [T][L][2][N] with the forward's sums sse [L][2] resp. the reverse sweep's g_sse
    // [L][2] and the forward's final state; `target` NULL: not a target form
    const float *target;
    double *sse;
    const double *g_sse;
    const float *fin_r, *fin_y, *fin_u;
    // on-ramps of the checkpointed pair and of the fused forward + tangent kernel: cells ramps [n_ramp] shared by all lanes, the density
    // rates inflow [T][L][n_ramp] and, reverse, their cotangent g_inflow [T][L][n_ramp]; `ramps` NULL: not a ramp form
    const int32_t *ramps;
    int n_ramp;
    const float *inflow;
    float *g_inflow;
};
static MacroForm macro_form(int ghost_is_sched, const int32_t *det = nullptr, int n_det = 0) {
    MacroForm f = {};
    f.bound = ghost_is_sched ? kBoundSched : kBoundConst; f.det = det; f.n_det = det ? n_det : 0;
    return f;
}
// ... and of the tape-free entry points, which also take a ring
static MacroForm macro_bound_form(MacroBoundary bound, const int32_t *det = nullptr, int n_det = 0) {
    MacroForm f = macro_form(0, det, n_det);
    f.bound = bound;
    return f;
}
// detectors and the array that goes with them (readings, their tangents or cotangents) come together or not at all
static inline bool macro_det_pair_ok(const dhts_macro_desc *d, const int32_t *det, int n_det, const void *with) {
    return (det != nullptr) == (with != nullptr) && (!det || (n_det >= 1 && n_det <= d->n_cells));
}

// T == 0 of every entry point but the constant-boundary rollout's: no step and no row of a schedule, of the tape or of the readings to
// address, so what the call carries through the steps comes back as it went in (what that rollout's kernel does with T = 0)
static bool macro_copy_back(void *dst, const void *src, size_t bytes, void *stream) {
    return dst == src || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess;
}
static int macro_state_copy(const dhts_macro_desc *d, const float *r, const float *y, const float *u, const float *ueq,
                            float *r_out, float *y_out, float *u_out, float *ueq_out, void *stream) {
    const size_t bytes = sizeof(float) * (size_t)d->n_lanes * d->n_cells;
    const float *src[4] = {r, y, u, ueq};
    float *dst[4] = {r_out, y_out, u_out, ueq_out};
    for (int k = 0; k < 4; ++k)
        if (!macro_copy_back(dst[k], src[k], bytes, stream)) return DHTS_E_LAUNCH;
    return DHTS_OK;
}

// The one-phase kernel.  kIface = false is the single-step operator's form (dqs-layout tape), which has neither a schedule nor taps.
static int macro_fwd_launch(bool iface, const dhts_macro_desc *d, int T,
                            const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                            float *r_out, float *y_out, float *u_out, float *ueq_out,
                            float *tape, const MacroForm &f, dhts_error *err, void *stream) {
    if (!macro_desc_ok(d) || T < 0 || !r || !y || !u || !ueq || !ghost || !r_out || !y_out || !u_out || !ueq_out)
        return DHTS_E_INVALID;
    const int N = d->n_cells;
    const size_t lds = sizeof(float) * 8 * (size_t)(N + 2);
    // Waves per lane: about 5 wavefronts on every SIMD of the chip (256 CUs x 4 SIMDs) when there are few lanes, 2 per lane
    // when there are many, at most 8, and never more than the lane has 63-cell chunks (p = passes per wave, chunk = 64 p - 1
    // cells).  Measured forward times in ms for waves per lane 1 / 2 / 3 / 5 / 8 (tools/sweep_fwd_waves.py, 1000 steps):
    //   4096 x 256: 13.3 / 12.5 / 12.6 / 14.3 / 14.1      2048 x 512: 15.1 / 10.9 / 11.8 / 12.5 / 12.6
    //   1024 x 512:  7.9 /  6.1 /  6.4 /  5.9 /  6.0       512 x 1000: 14.4 / 10.2 /  7.9 /  5.2 /  4.7
    //    256 x 2048: 27.6 / 14.9 /  9.6 /  7.0 /  6.5
    int W = dhts_fwd_waves_override > 0 ? dhts_fwd_waves_override
                                        : (d->n_lanes >= 1536 ? 2 : (int)((5 * 1024 + d->n_lanes - 1) / d->n_lanes));
    if (W > 8) W = 8;
    if (W < 1) W = 1;
    int p = 1;
    while ((N + (64 * p - 1) - 1) / (64 * p - 1) > W) ++p;
    W = (N + (64 * p - 1) - 1) / (64 * p - 1);
    bool lds_ok = true;
    pick<1, 0>(iface, [&](auto fc) {
        pick<0, 1>(f.sched(), [&](auto sc) {
            pick<0, 1>(f.det != nullptr, [&](auto tp) {
                constexpr bool kIface = decltype(fc)::value != 0, kS = decltype(sc)::value != 0, kT = decltype(tp)::value != 0;
                if constexpr (kIface || (!kS && !kT))
                    lds_ok = launch_lds(macro_rollout_fwd_kernel<kIface, kS, kT>, d->n_lanes, 64 * W, lds, kLdsDefault, stream, d->n_lanes, N, T, p,
                                        d->dt, d->dx, d->u_max, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out,
                                        reinterpret_cast<float4 *>(tape), f.hist, err, f.det, f.n_det, f.taps);
            });
        });
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

// The forward rollout of every form: the plan names the kernel and its shape arguments, the form its kSched and kTaps.
static int macro_rollout_fwd_launch(const dhts_macro_desc *d, int T,
                                    const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                    float *r_out, float *y_out, float *u_out, float *ueq_out,
                                    float *tape, const MacroForm &f, dhts_error *err, void *stream) {
    const MacroPlan pl = macro_plan(d, T, f.hist != nullptr, tape != nullptr, f.det != nullptr);
    if (pl.fwd == kMacroFwdOnePhase) return macro_fwd_launch(true, d, T, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out, tape, f, err, stream);
    const int N = d->n_cells;
    float4 *tp = reinterpret_cast<float4 *>(tape);
    bool lds_ok = true;
    pick<0, 1>(f.sched(), [&](auto sc) {
        pick<0, 1>(f.det != nullptr, [&](auto tap) {
            constexpr bool kS = decltype(sc)::value != 0, kT = decltype(tap)::value != 0;
            if (pl.fwd == kMacroFwdLane) {
                // <kP, kFull, kHist> as 10 kP + kFull (kHist = !kFull, with detectors too: `hist` is NULL then); kP = 0: the run-time
                // pass count
                pick<0, 20, 10, 21, 11>(10 * (pl.p <= 2 ? pl.p : 0) + (pl.dense ? 1 : 0), [&](auto v) {
                    constexpr int kV = decltype(v)::value;
                    lds_ok = launch_lds(macro_rollout_fwd2_kernel<kV / 10, kV % 10 != 0, kV % 10 == 0, kS, kT>, d->n_lanes, 64 * pl.W, pl.lds_fwd,
                                        kLdsDefault, stream, d->n_lanes, N, T, pl.p, d->dt, d->dx, d->u_max, r, y, u, ueq, ghost, r_out, y_out, u_out,
                                        ueq_out, tp, f.hist, err, f.det, f.n_det, f.taps);
                });
            } else {
                // the pair kernel: a thread owns two adjacent cells and their right interfaces (macro_fwd_pairs.inc)
                pick<4, 2, 1>(pl.G, [&](auto g) {
                    pick<0, 1>(pl.tape, [&](auto tp_) {
                        constexpr int kG = decltype(g)::value;
                        lds_ok = launch_lds(macro_rollout_fwd3_kernel<kG, decltype(tp_)::value != 0, kS, kT>, d->n_lanes / kG, 64 * kG * (N / 128),
                                            pl.lds_fwd, kLdsDefault, stream, d->n_lanes, N, T, d->dt, d->dx, d->u_max, r, y, u, ueq, ghost, r_out,
                                            y_out, u_out, ueq_out, tp, err, dhts_fwd_rotate, f.det, f.n_det, f.taps);
                    });
                });
            }
        });
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

static int macro_blocks_bwd_launch(const dhts_macro_desc *d, int T, const float *tape,
                                  const float *g_r, const float *g_y, const float *g_hist,
                                  float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream) {
    if (!macro_desc_ok(d) || T < 0 || (T > 0 && !tape) || !g_r || !g_y || !g_r_out || !g_y_out) return DHTS_E_INVALID;
    const size_t lds = sizeof(float) * 6 * (size_t)(d->n_cells + 2);
    int B = padded64(d->n_cells);
    if (B > 512) B = 512;
    if (!launch_lds(macro_blocks_bwd_kernel, d->n_lanes, B, lds, kLdsDefault, stream, d->n_lanes, d->n_cells, T,
                    reinterpret_cast<const float4 *>(tape), g_r, g_y, g_hist, g_r_out, g_y_out, g_ghost, err))
        return DHTS_E_LAUNCH;
    return launch_status();
}

// The reverse sweep of every form, as above.
static int macro_rollout_bwd_launch(const dhts_macro_desc *d, int T, const float *tape, const float *g_r, const float *g_y,
                                    float *g_r_out, float *g_y_out, double *g_ghost, const MacroForm &f, dhts_error *err, void *stream) {
    if (!macro_desc_ok(d) || T < 0 || (T > 0 && !tape) || !g_r || !g_y || !g_r_out || !g_y_out || (f.sched() && !g_ghost)) return DHTS_E_INVALID;
    const MacroPlan pl = macro_plan(d, T, f.g_cot != nullptr && !f.det, tape != nullptr, f.det != nullptr);
    const int N = d->n_cells, B = pl.bwd_block;
    const float4 *tp = reinterpret_cast<const float4 *>(tape);
    const double cc = d->dt / d->dx;
    if (pl.lds_bwd > 160 * 1024) return DHTS_E_INVALID;
    bool lds_ok = true;
    pick<0, 1>(f.sched(), [&](auto sc) {
        pick<0, 1>(f.det != nullptr, [&](auto tap) {
            constexpr bool kS = decltype(sc)::value != 0, kT = decltype(tap)::value != 0;
            if (pl.bwd == kMacroBwdFast) {
                // <kB, kHist, kFull> as 10 kB + (0 plain, 1 kHist, 2 kFull): every combination a plan can name (kFull: 128 <= N = kB <= 512).
                // Detectors exclude the dense per-step cotangents (the plan of the taps form has no history).
                pick<5120, 5122, 5121, 2560, 2562, 2561, 1280, 1282, 1281, 640, 641, 10241, 10240>(
                    10 * B + (pl.hist ? 1 : (pl.bwd_full ? 2 : 0)), [&](auto v) {
                        constexpr int kV = decltype(v)::value;
                        if constexpr (!(kT && kV % 10 == 1))
                            lds_ok = launch_lds(macro_rollout_bwd_fast_kernel<kV / 10, kV % 10 == 1, kV % 10 == 2, kS, kT>, d->n_lanes, B, pl.lds_bwd,
                                                kLdsDefault, stream, d->n_lanes, N, T, cc, tp, g_r, g_y, f.g_cot, g_r_out, g_y_out, g_ghost, err,
                                                f.det, f.n_det);
                    });
            } else if (pl.bwd == kMacroBwdFast2) {
                // two cells per thread: no per-step cotangents, so no detector form (the plan sends that to the general sweep)
                if constexpr (!kT)
                    pick<0, 1>(pl.bwd_full, [&](auto full) {
                        lds_ok = launch_lds(macro_rollout_bwd_fast2_kernel<1024, decltype(full)::value != 0, kS>, d->n_lanes, B, pl.lds_bwd,
                                            kLdsDefault, stream, d->n_lanes, N, T, cc, tp, g_r, g_y, g_r_out, g_y_out, g_ghost, err);
                    });
            } else {
                lds_ok = launch_lds(macro_rollout_bwd_kernel<kS, kT>, d->n_lanes, B, pl.lds_bwd, kLdsDefault, stream, d->n_lanes, N, T, cc, tp, g_r,
                                    g_y, f.g_cot, g_r_out, g_y_out, g_ghost, err, f.det, f.n_det);
            }
        });
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

// The tangent sweep (macro_jvp.inc): which kernel a shape takes, how many directions ride in one launch and how many launches n_dir
// directions need.  Launches of 4, then 2, then 1 directions; a remainder of 3 runs as ONE launch of 4 with a slot masked (the tape is
// read once instead of twice: jvp_width, host_common.hpp); lanes too long for the general kernel's LDS at 4 directions (two plane sets per direction) take fewer.
struct JvpPlan {
    bool fast;
    int block;            // threads per lane
    int kmax;             // directions a launch may carry: 4, 2 or 1 (0: not even one fits)
    int widest, launches; // of n_dir directions: the slots of the widest launch, the number of launches
};
static JvpPlan macro_jvp_plan(const dhts_macro_desc *d, int T, int n_dir) {
    JvpPlan pl = {};
    const int N = d->n_cells;
    pl.fast = dhts_jvp_variant == 0 && N >= 2 && N <= 1024 && T > 0;       // (T = 0: no tape to prefetch from, and nothing is launched)
    pl.kmax = 4;
    if (pl.fast) {
        pl.block = N <= 64 ? 64 : (N <= 128 ? 128 : (N <= 256 ? 256 : (N <= 512 ? 512 : 1024)));
    } else {
        pl.block = padded64(N) > 512 ? 512 : padded64(N);
        while (pl.kmax > 0 && jvp_general_lds_bytes(N, pl.kmax) > 160 * 1024) pl.kmax >>= 1;
    }
    const JvpGroups g = jvp_groups(pl.kmax, n_dir);
    pl.widest = g.widest;
    pl.launches = T == 0 ? 0 : g.launches;      // (T = 0: nothing to sweep, the entry point copies the tangents)
    return pl;
}

// The per-direction arrays of the two tangent entry points, [K] outermost: the tangents of (r, y) in and out, t_ghost [K][L][2][2] or
// beside a schedule [K][T][L][2][2] (NULL: zero), the tangent readings [K][T][L][2][n_det] (with detectors).  ..._at: those of one
// launch, which starts at direction k0.  inflow: the fused kernel's ramp forms alone -- the tangents of f.inflow, [K][T][L][n_ramp] (NULL: zero).
struct MacroTangents {
    const float *r, *y, *ghost;
    float *r_out, *y_out, *taps;
    const float *inflow;
};
static MacroTangents macro_tangents_at(const MacroTangents &t, int k0, const dhts_macro_desc *d, int T, const MacroForm &f) {
    const size_t dir_state = (size_t)d->n_lanes * d->n_cells, dir_ghost = (f.sched() ? (size_t)T : 1) * d->n_lanes * 4,
                 dir_taps = (size_t)T * d->n_lanes * 2 * f.n_det, dir_inflow = (size_t)T * d->n_lanes * f.n_ramp;
    return {t.r + k0 * dir_state, t.y + k0 * dir_state, t.ghost ? t.ghost + k0 * dir_ghost : nullptr,
            t.r_out + k0 * dir_state, t.y_out + k0 * dir_state, f.det ? t.taps + k0 * dir_taps : nullptr,
            f.ramps && t.inflow ? t.inflow + k0 * dir_inflow : nullptr};
}
// how the kernels read t_ghost: 0 none, 1 the same in front of every step, 2 a schedule
static int macro_ghost_mode(const MacroTangents &t, const MacroForm &f) { return !t.ghost ? 0 : (f.sched() ? 2 : 1); }
// T == 0 of both: the tangents come back as they went in, no row is read or written
static bool macro_tangents_copy(const dhts_macro_desc *d, int n_dir, const MacroTangents &t, void *stream) {
    const size_t bytes = sizeof(float) * (size_t)n_dir * d->n_lanes * d->n_cells;
    return macro_copy_back(t.r_out, t.r, bytes, stream) && macro_copy_back(t.y_out, t.y, bytes, stream);
}

static int macro_rollout_jvp_launch(const dhts_macro_desc *d, int T, const float *tape, int n_dir, const MacroTangents &t, const MacroForm &f,
                                    dhts_error *err, void *stream) {
    const JvpPlan pl = macro_jvp_plan(d, T, n_dir);
    if (pl.kmax < 1) return DHTS_E_INVALID;
    const int L = d->n_lanes, N = d->n_cells, B = pl.block;
    const float4 *tp = reinterpret_cast<const float4 *>(tape);
    const double cc = d->dt / d->dx;
    const int ghost_mode = macro_ghost_mode(t, f);
    const bool lds_ok = jvp_each_group(n_dir, pl.kmax, [&](int k0, auto kv, int n_act) {
        constexpr int kK = decltype(kv)::value;
        const MacroTangents a = macro_tangents_at(t, k0, d, T, f);
        bool ok = true;
        if (pl.fast) {
            pick<64, 128, 256, 512, 1024>(B, [&](auto bv) {
                constexpr int kB = decltype(bv)::value;
                ok = launch_lds(macro_rollout_jvp_fast_kernel<kB, kK>, L, B, jvp_fast_lds_bytes(kB, kK), kLdsDefault, stream, L, N, T, cc, tp, a.r,
                                a.y, a.ghost, ghost_mode, n_act, a.r_out, a.y_out, f.det, f.n_det, a.taps, err);
            });
        } else {
            ok = launch_lds(macro_rollout_jvp_kernel<kK>, L, B, jvp_general_lds_bytes(N, kK), kLdsDefault, stream, L, N, T, cc, tp, a.r, a.y,
                            a.ghost, ghost_mode, n_act, a.r_out, a.y_out, f.det, f.n_det, a.taps, err);
        }
        return ok;
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

// The tape-free fused forward + tangent kernel (macro_fwd_jvp.inc): the lane kernel's mapping (W wavefronts of p passes, computed as
// macro_plan computes them for the two-phase lane kernel; DHTS_OPT_MACRO_FWD_VARIANT and _GROUP do not apply: there is one kernel) and the
// widest launch whose dynamic LDS -- the lane kernel's records, the interface products, two tangent copies per direction -- fits 160 KB:
// 4 directions up to 997 cells, 2 up to 1239, 1 up to 1410, none above (kmax = 0: the taped pair covers those lanes).
struct FwdJvpPlan {
    int W, p;             // wavefronts per lane, 64-cell passes per wavefront
    int kmax;             // directions a launch may carry: 4, 2, 1 or 0
    int widest, launches; // of n_dir directions: the slots of the widest launch, the number of launches
    size_t lds;           // dynamic LDS of the widest launch
};
static FwdJvpPlan macro_fwd_jvp_plan(const dhts_macro_desc *d, int T, int n_dir) {
    FwdJvpPlan pl = {};
    const int N = d->n_cells;
    // (12: the kernel's launch bound; no lane that fits has more without DHTS_OPT_MACRO_FWD_WAVES)
    const MacroLaneMap m = macro_lane_map(N, dhts_fwd_waves_override > 0 ? dhts_fwd_waves_override : (N + 127) / 128, 12);
    pl.W = m.W; pl.p = m.p;
    pl.kmax = 4;
    while (pl.kmax > 0 && fwd_jvp_lds_bytes(N, pl.kmax) > 160 * 1024) pl.kmax >>= 1;
    const JvpGroups g = jvp_groups(pl.kmax, n_dir);
    pl.widest = g.widest;
    pl.launches = T == 0 ? 0 : g.launches;      // (T = 0: no step, the entry point copies the state and the tangents)
    pl.lds = pl.widest > 0 ? fwd_jvp_lds_bytes(N, pl.widest) : 0;
    return pl;
}

// f.taps: the primal readings; t.taps: their tangents
static int macro_fwd_jvp_launch(const dhts_macro_desc *d, int T, int n_dir, const float *r, const float *y, const float *u, const float *ueq,
                                const float *ghost, const MacroTangents &t, float *r_out, float *y_out, float *u_out, float *ueq_out,
                                const MacroForm &f, dhts_error *err, dhts_error *err_jvp, void *stream) {
    const FwdJvpPlan pl = macro_fwd_jvp_plan(d, T, n_dir);
    if (pl.kmax < 1) return DHTS_E_INVALID;
    const int L = d->n_lanes, N = d->n_cells;
    const int ghost_mode = macro_ghost_mode(t, f);
    const bool lds_ok = jvp_each_group(n_dir, pl.kmax, [&](int k0, auto kv, int n_act) {
        const MacroTangents a = macro_tangents_at(t, k0, d, T, f);
        // every launch recomputes the primal and writes the same bits; the first one alone is handed the readings and the forward's record
        float *o_taps = k0 == 0 ? f.taps : nullptr;
        dhts_error *o_err = k0 == 0 ? err : nullptr;
        bool ok = true;
        pick<0, 1, 2>(pl.p <= 2 ? pl.p : 0, [&](auto pv) {
            pick<kBoundConst, kBoundSched, kBoundRing>(f.bound, [&](auto bc) {
                pick<0, 1>(f.det != nullptr, [&](auto tap) {
                    pick<0, 1>(f.ramps != nullptr, [&](auto ramp) {
                        constexpr int kK = decltype(kv)::value, kP = decltype(pv)::value;
                        constexpr MacroBoundary kS = (MacroBoundary) decltype(bc)::value;
                        constexpr bool kT = decltype(tap)::value != 0, kR = decltype(ramp)::value != 0;
                        ok = launch_lds(macro_rollout_fwd_jvp_kernel<kK, kP, kS, kT, kR>, L, 64 * pl.W, fwd_jvp_lds_bytes(N, kK), kLdsDefault,
                                        stream, L, N, T, pl.p, d->dt, d->dx, d->u_max, r, y, u, ueq, ghost, a.r, a.y, a.ghost, ghost_mode, n_act,
                                        r_out, y_out, u_out, ueq_out, a.r_out, a.y_out, f.det, f.n_det, o_taps, a.taps, o_err, err_jvp, f.ramps,
                                        f.n_ramp, f.inflow, a.inflow);
                    });
                });
            });
        });
        return ok;
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

// The checkpointed pair (macro_ckpt.inc): the lane kernel's mapping for both kernels (W wavefronts of p passes as macro_plan computes them
// for the two-phase lane kernel, at most 12 wavefronts; DHTS_OPT_MACRO_FWD_WAVES, _VARIANT and _GROUP do not apply: there is one kernel
// pair, and every lane it takes has p = 1 or 2), the longest segment whose reverse LDS -- parked pointers, records, planes, one ring entry per step -- fits
// kMacroCkptLdsBudget (0: not even one step fits, 1320 cells and above; the taped pair covers those lanes) and the segment a caller gets
// who names none.  A pure function of the lane length: the two launches, dhts_macro_ckpt_plan and dhts_macro_ckpt_bytes read it.
// The default segment is 4e's rule with this kernel's numbers: the longest, up to kMacroCkptSegmentCap, whose reverse workgroup still
// leaves the residency the sweep needs to hide its barrier chain (replay and sweep are barrier chains: what hides them is another
// workgroup).  That residency is kMacroCkptWavesPerCu = 12 wavefronts on a CU -- three per SIMD, all the reverse kernel's registers
// admit --, or, for lanes whose LDS does not reach it even with a one-step ring, the workgroups per CU a one-step ring has.  Measured
// (DESIGN 4f): the fastest pair at 1024 x 512 (S = 2 of 1 .. 7) and at 4096 x 64 (S = 3 of 1 .. 75) is the one this picks.
constexpr size_t kMacroCkptLdsBudget = 160 * 1024;      // LDS of a CU: what one workgroup may take
constexpr int kMacroCkptSegmentCap = 16;
constexpr int kMacroCkptWavesPerCu = 12;
struct MacroCkptPlan {
    int W, p;             // wavefronts per lane, 64-cell passes per wavefront
    int segment;          // the plan's own segment length
    int max_segment;      // the longest one the reverse kernel's LDS holds; 0: the lane does not fit
    size_t lds_fwd;
};
// target: the plan of the target forms (dhts_macro_ckpt_target_plan), whose ring step is two float planes wider: the same rule
static MacroCkptPlan macro_ckpt_plan(const dhts_macro_desc *d, bool target = false) {
    MacroCkptPlan pl = {};
    const int N = d->n_cells;
    const MacroLaneMap m = macro_lane_map(N, (N + 127) / 128, 12);
    pl.W = m.W; pl.p = m.p;
    pl.lds_fwd = macro_ckpt_fwd_lds_bytes(N);
    const size_t fixed = macro_ckpt_bwd_fixed_bytes(N), step = macro_ckpt_bwd_step_bytes(N, target);
    pl.max_segment = fixed + step <= kMacroCkptLdsBudget && pl.p <= 2 ? (int)((kMacroCkptLdsBudget - fixed) / step) : 0;
    const int by_regs = (kMacroCkptWavesPerCu + pl.W - 1) / pl.W;               // workgroups per CU that make kMacroCkptWavesPerCu
    const int at_one = (int)(kMacroCkptLdsBudget / (fixed + step));             // ... that a one-step ring leaves
    const int groups = at_one < 1 ? 1 : (by_regs < at_one ? by_regs : at_one);
    const long long room = (long long)(kMacroCkptLdsBudget / groups) - (long long)fixed;
    int S = room > 0 ? (int)(room / (long long)step) : 0;
    S = S > kMacroCkptSegmentCap ? kMacroCkptSegmentCap : S;
    S = S < 1 ? 1 : S;
    pl.segment = S > pl.max_segment ? pl.max_segment : S;
    return pl;
}
// the segment a call runs with: `segment` itself, the plan's for 0; -1: outside 0 .. max_segment, or the lane does not fit
static int macro_ckpt_segment(const MacroCkptPlan &pl, int segment) {
    if (pl.max_segment < 1 || segment < 0 || segment > pl.max_segment) return -1;
    return segment == 0 ? pl.segment : segment;
}
static int macro_ckpt_count(int T, int S) { return T > 0 ? (T + S - 1) / S : 0; }
// what dhts_macro_ckpt_plan and dhts_macro_ckpt_target_plan answer, each after its own argument check
static int macro_ckpt_plan_fill(const dhts_macro_desc *d, int T, int segment, bool target, int32_t plan[8]) {
    const MacroCkptPlan pl = macro_ckpt_plan(d, target);
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = pl.W; plan[1] = pl.p; plan[3] = pl.max_segment; plan[5] = (int32_t)pl.lds_fwd;
    if (pl.max_segment < 1) return segment == 0 ? DHTS_OK : DHTS_E_INVALID;       // the lane does not fit: max_segment = 0 says so
    const int S = macro_ckpt_segment(pl, segment);
    if (S < 0) return DHTS_E_INVALID;
    const size_t bwd_lds = macro_ckpt_bwd_lds_bytes(d->n_cells, S, target);
    plan[2] = S;
    plan[4] = macro_ckpt_count(T, S);
    plan[6] = (int32_t)bwd_lds;
    plan[7] = (int32_t)(kMacroCkptLdsBudget / bwd_lds);
    return DHTS_OK;
}

// f.target: the target kernels (f.sse resp. f.g_sse and the final state); else f.det with f.taps resp. the cotangents f.g_cot, or neither
static int macro_ckpt_fwd_launch(const dhts_macro_desc *d, int T, int S, const MacroCkptPlan &pl,
                                 const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                 float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt, const MacroForm &f, dhts_error *err,
                                 void *stream) {
    const int L = d->n_lanes, N = d->n_cells;
    bool lds_ok = true;
    auto go = [&](auto kernel, auto... tail) {
        lds_ok = launch_lds(kernel, L, 64 * pl.W, pl.lds_fwd, kLdsDefault, stream, L, N, T, S, d->dt, d->dx, d->u_max, r, y, u, ueq, ghost, r_out,
                            y_out, u_out, ueq_out, reinterpret_cast<float2 *>(ckpt), err, tail...);
    };
    pick<1, 2>(pl.p, [&](auto pv) {
        pick<kBoundConst, kBoundSched, kBoundRing>(f.bound, [&](auto bc) {
            pick<0, 1, 2>(f.target ? 2 : f.det != nullptr, [&](auto tap) {
                pick<0, 1>(f.ramps != nullptr, [&](auto rv) {
                    constexpr int kP = decltype(pv)::value, kForm = decltype(tap)::value;
                    constexpr MacroBoundary kS = (MacroBoundary) decltype(bc)::value;
                    constexpr bool kR = decltype(rv)::value != 0;
                    if constexpr (kForm == 2) go(macro_rollout_ckpt_fwd_target_kernel<kP, kS, kR>, f.target, f.sse, f.ramps, f.n_ramp, f.inflow);
                    else go(macro_rollout_ckpt_fwd_kernel<kP, kS, kForm != 0, kR>, f.det, f.n_det, f.taps, f.ramps, f.n_ramp, f.inflow);
                });
            });
        });
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}
static int macro_ckpt_bwd_launch(const dhts_macro_desc *d, int T, int S, const MacroCkptPlan &pl, const void *ckpt,
                                 const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                 const float *g_r, const float *g_y, float *g_r_out, float *g_y_out, double *g_ghost, const MacroForm &f,
                                 dhts_error *err, void *stream) {
    const int L = d->n_lanes, N = d->n_cells;
    bool lds_ok = true;
    auto go = [&](auto kernel, size_t lds, auto... tail) {
        lds_ok = launch_lds(kernel, L, 64 * pl.W, lds, kLdsDefault, stream, L, N, T, S, pl.p, d->dt, d->dx, d->u_max,
                            reinterpret_cast<const float2 *>(ckpt), r, y, u, ueq, ghost, g_r, g_y, f.g_cot, g_r_out, g_y_out, g_ghost, err, tail...);
    };
    pick<kBoundConst, kBoundSched, kBoundRing>(f.bound, [&](auto bc) {
        pick<0, 1, 2>(f.target ? 2 : f.det != nullptr, [&](auto tap) {
            pick<0, 1>(f.ramps != nullptr, [&](auto rv) {
                constexpr MacroBoundary kS = (MacroBoundary) decltype(bc)::value;
                constexpr int kForm = decltype(tap)::value;
                constexpr bool kR = decltype(rv)::value != 0;
                if constexpr (kForm == 2)
                    go(macro_rollout_ckpt_bwd_target_kernel<kS, kR>, macro_ckpt_bwd_lds_bytes(N, S, true), f.target, f.g_sse, f.fin_r, f.fin_y,
                       f.fin_u, f.ramps, f.n_ramp, f.inflow, f.g_inflow);
                else
                    go(macro_rollout_ckpt_bwd_kernel<kS, kForm != 0, kR>, macro_ckpt_bwd_lds_bytes(N, S), f.det, f.n_det, f.ramps, f.n_ramp, f.inflow,
                       f.g_inflow);
            });
        });
    });
    return lds_ok ? launch_status() : DHTS_E_LAUNCH;
}

#ifdef DHTS_FWD3_STAMPS
extern "C" int dhts_debug_fwd_clock(long long *out) {         // [2 kernels][16 workgroups][2]
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(dhts::dhts_fwd_clock), sizeof(long long) * 2 * 16 * 2) == hipSuccess ? 0 : -1;
}
extern "C" int dhts_debug_fwd3_stamps(long long *out) {       // [16 workgroups][16 wavefronts][8], macro_fwd_pairs.inc
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(dhts::dhts_fwd3_stamps), sizeof(long long) * 16 * 16 * 8) == hipSuccess ? 0 : -1;
}
#endif

extern "C" {

size_t dhts_macro_tape_bytes(const dhts_macro_desc *d, int T) {
    if (!macro_desc_ok(d) || T < 0) return 0;
    return (size_t)T * d->n_lanes * tape_geom(d->n_cells).row_f4 * sizeof(float4);
}
size_t dhts_macro_step_tape_bytes(const dhts_macro_desc *d) {
    if (!macro_desc_ok(d)) return 0;
    return (size_t)d->n_lanes * 3 * padded64(d->n_cells) * sizeof(float4);
}

int dhts_arz_interface_batch(int64_t n, int variant, const double *in, double dt, double dx, int32_t *case_ind, double *q0,
                             double *flux, float *dL, float *dR, float *fp, float *A, float *B, int32_t *cfl_bad, double *speed,
                             void *stream) {
    if (n < 0 || (variant != 0 && variant != 1) || !in || !case_ind || !q0 || !flux || !dL || !dR || !fp || !A || !B || !cfl_bad)
        return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(arz_interface_batch_kernel, grid_1d(n), 256, 0, stream, n, variant, in, dt, dx, case_ind, q0, flux, dL, dR, fp,
                                                                          A, B, cfl_bad, speed);
    return launch_status();
}

int dhts_macro_state_from_ru(int64_t n, double u_max, const float *r, const float *u, float *y, float *ueq, void *stream) {
    if (n < 0 || !r || !u || !y || !ueq) return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(macro_state_from_ru_kernel, grid_1d(n), 256, 0, stream, n, (float)u_max, r, u, y, ueq);
    return launch_status();
}
int dhts_macro_state_from_ru_bwd(int64_t n, double u_max, const float *r, const float *u, const float *g_y,
                                 float *g_r, float *g_u, void *stream) {
    if (n < 0 || !r || !u || !g_y || !g_r || !g_u) return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(macro_state_from_ru_bwd_kernel, grid_1d(n), 256, 0, stream, n, (float)u_max, r, u, g_y, g_r, g_u);
    return launch_status();
}
int dhts_macro_u_tap_bwd(int64_t n, double u_max, const float *r, const float *y, const float *g_u,
                         float *g_r, float *g_y, void *stream) {
    if (n < 0 || !r || !y || !g_u || !g_r || !g_y) return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(macro_u_tap_bwd_kernel, grid_1d(n), 256, 0, stream, n, (float)u_max, r, y, g_u, g_r, g_y);
    return launch_status();
}

// rollouts keep the compact tape described above (three floats per trivial interface + the exceptions' products)
static inline bool macro_fwd_args_ok(const dhts_macro_desc *d, int T, const float *r, const float *y, const float *u, const float *ueq,
                                     const float *ghost, const float *r_out, const float *y_out, const float *u_out, const float *ueq_out) {
    return macro_desc_ok(d) && T >= 0 && r && y && u && ueq && ghost && r_out && y_out && u_out && ueq_out;
}
int dhts_macro_rollout_fwd(const dhts_macro_desc *d, int T,
                           const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                           float *r_out, float *y_out, float *u_out, float *ueq_out,
                           float *tape, float *hist, dhts_error *err, void *stream) {
    if (!macro_fwd_args_ok(d, T, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out)) return DHTS_E_INVALID;
    MacroForm f = {};
    f.hist = hist;
    return macro_rollout_fwd_launch(d, T, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out, tape, f, err, stream);
}
int dhts_macro_rollout_bwd(const dhts_macro_desc *d, int T, const float *tape,
                           const float *g_r, const float *g_y, const float *g_hist,
                           float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream) {
    MacroForm f = {};
    f.g_cot = g_hist;
    return macro_rollout_bwd_launch(d, T, tape, g_r, g_y, g_r_out, g_y_out, g_ghost, f, err, stream);
}
// the same rollout with a boundary schedule: the same plan, the kSched instantiation of the kernel it names
int dhts_macro_rollout_fwd_sched(const dhts_macro_desc *d, int T,
                                 const float *r, const float *y, const float *u, const float *ueq, const float *ghost_sched,
                                 float *r_out, float *y_out, float *u_out, float *ueq_out,
                                 float *tape, float *hist, dhts_error *err, void *stream) {
    if (!macro_fwd_args_ok(d, T, r, y, u, ueq, ghost_sched, r_out, y_out, u_out, ueq_out)) return DHTS_E_INVALID;
    if (T == 0) return macro_state_copy(d, r, y, u, ueq, r_out, y_out, u_out, ueq_out, stream);
    MacroForm f = macro_form(true);
    f.hist = hist;
    return macro_rollout_fwd_launch(d, T, r, y, u, ueq, ghost_sched, r_out, y_out, u_out, ueq_out, tape, f, err, stream);
}
int dhts_macro_rollout_bwd_sched(const dhts_macro_desc *d, int T, const float *tape,
                                 const float *g_r, const float *g_y, const float *g_hist,
                                 float *g_r_out, float *g_y_out, double *g_ghost_sched, dhts_error *err, void *stream) {
    MacroForm f = macro_form(true);
    f.g_cot = g_hist;
    return macro_rollout_bwd_launch(d, T, tape, g_r, g_y, g_r_out, g_y_out, g_ghost_sched, f, err, stream);
}
// the rollout with detector taps instead of a history (constant boundary cells or a schedule): the plan of the same shape without a
// history, the kTaps instantiation of the kernel it names
static inline bool macro_taps_ok(const dhts_macro_desc *d, const int32_t *det, int n_det) {
    return macro_desc_ok(d) && det && n_det >= 1 && n_det <= d->n_cells;
}
int dhts_macro_rollout_fwd_taps(const dhts_macro_desc *d, int T,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                float *r_out, float *y_out, float *u_out, float *ueq_out, float *tape,
                                const int32_t *det, int n_det, float *taps, dhts_error *err, void *stream) {
    if (!macro_taps_ok(d, det, n_det) || !taps || !macro_fwd_args_ok(d, T, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out))
        return DHTS_E_INVALID;
    if (T == 0) return macro_state_copy(d, r, y, u, ueq, r_out, y_out, u_out, ueq_out, stream);
    MacroForm f = macro_form(ghost_is_sched, det, n_det);
    f.taps = taps;
    return macro_rollout_fwd_launch(d, T, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out, tape, f, err, stream);
}
int dhts_macro_rollout_bwd_taps(const dhts_macro_desc *d, int T, const float *tape, const float *g_r, const float *g_y,
                                const int32_t *det, int n_det, const float *g_taps,
                                float *g_r_out, float *g_y_out, double *g_ghost, int ghost_is_sched, dhts_error *err, void *stream) {
    if (!macro_taps_ok(d, det, n_det) || !g_taps) return DHTS_E_INVALID;
    MacroForm f = macro_form(ghost_is_sched, det, n_det);
    f.g_cot = g_taps;
    return macro_rollout_bwd_launch(d, T, tape, g_r, g_y, g_r_out, g_y_out, g_ghost, f, err, stream);
}
// which kernel instantiations the rollout entry points launch for a shape: the plan the launches read, as include/dhts.h lays it out
static int macro_plan_out(const MacroPlan &pl, int32_t plan[8]) {
    plan[0] = pl.fwd; plan[1] = pl.W; plan[2] = pl.p; plan[3] = pl.dense ? 1 : 0;
    plan[4] = pl.bwd; plan[5] = pl.bwd_block; plan[6] = pl.hist ? 1 : 0; plan[7] = pl.G;
    return DHTS_OK;
}
int dhts_macro_taps_plan(const dhts_macro_desc *d, int T, int n_det, int32_t plan[8]) {
    if (!macro_desc_ok(d) || T < 0 || !plan || n_det < 1 || n_det > d->n_cells) return DHTS_E_INVALID;
    return macro_plan_out(macro_plan(d, T, false, true, true), plan);       // (no history: plan[6] = 0)
}
int dhts_macro_rollout_plan(const dhts_macro_desc *d, int T, int want_hist, int32_t plan[8]) {       // (the _sched forms too)
    if (!macro_desc_ok(d) || T < 0 || !plan) return DHTS_E_INVALID;
    return macro_plan_out(macro_plan(d, T, want_hist != 0, true), plan);
}
int dhts_macro_tape_expand(const dhts_macro_desc *d, int T, const float *tape, float *dqs, void *stream) {
    if (!macro_desc_ok(d) || T < 0 || (T > 0 && (!tape || !dqs))) return DHTS_E_INVALID;
    if (T == 0) return DHTS_OK;
    const size_t lds = 2 * (size_t)(d->n_cells + 1);
    launch(macro_tape_expand_kernel, (unsigned)((size_t)T * d->n_lanes), 256, lds, stream, d->n_cells, d->dt / d->dx,
           reinterpret_cast<const float4 *>(tape), reinterpret_cast<float4 *>(dqs));
    return launch_status();
}
// the single-step operator keeps the reference's per-cell blocks dqs[a][3][2][2] (48 B per cell)
int dhts_macro_step_fwd(const dhts_macro_desc *d,
                        const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                        float *r_out, float *y_out, float *u_out, float *ueq_out,
                        float *tape, dhts_error *err, void *stream) {
    return macro_fwd_launch(false, d, 1, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out, tape, MacroForm{}, err, stream);
}
int dhts_macro_step_bwd(const dhts_macro_desc *d, const float *tape, const float *g_r, const float *g_y,
                        float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream) {
    return macro_blocks_bwd_launch(d, 1, tape, g_r, g_y, nullptr, g_r_out, g_y_out, g_ghost, err, stream);
}

// ---- the tangent sweep ----------------------------------------------------------------------------------------------------------
int dhts_macro_rollout_jvp(const dhts_macro_desc *d, int T, const float *tape, int n_dir, const float *t_r, const float *t_y,
                           const float *t_ghost, int ghost_is_sched, float *t_r_out, float *t_y_out,
                           const int32_t *det, int n_det, float *t_taps, dhts_error *err, void *stream) {
    if (!macro_desc_ok(d) || T < 0 || n_dir < 1 || (T > 0 && !tape) || !t_r || !t_y || !t_r_out || !t_y_out) return DHTS_E_INVALID;
    if (!macro_det_pair_ok(d, det, n_det, t_taps)) return DHTS_E_INVALID;
    if (ghost_is_sched && !t_ghost) return DHTS_E_INVALID;       // a schedule that is not there (zero boundary tangents: NULL with 0)
    const MacroTangents t = {t_r, t_y, t_ghost, t_r_out, t_y_out, t_taps};
    if (T == 0) return macro_tangents_copy(d, n_dir, t, stream) ? DHTS_OK : DHTS_E_LAUNCH;
    return macro_rollout_jvp_launch(d, T, tape, n_dir, t, macro_form(ghost_is_sched, det, n_det), err, stream);
}
int dhts_macro_jvp_plan(const dhts_macro_desc *d, int T, int n_dir, int n_det, int32_t plan[8]) {
    if (!macro_desc_ok(d) || T < 0 || n_dir < 1 || !plan || n_det < 0 || n_det > d->n_cells) return DHTS_E_INVALID;
    const JvpPlan pl = macro_jvp_plan(d, T, n_dir);
    if (pl.kmax < 1) return DHTS_E_INVALID;
    plan[0] = pl.fast ? 1 : 0; plan[1] = pl.block; plan[2] = pl.widest; plan[3] = pl.launches;
    plan[4] = plan[5] = plan[6] = plan[7] = 0;
    return DHTS_OK;
}
// ---- the rollout and its tangents in one kernel, no tape ------------------------------------------------------------------------
// (the bodies of the tape-free entry points take the form's boundary: of a ring, `ghost`, t_ghost and g_ghost are NULL and nothing is
// asked of them -- ring_or(bound, r, ghost) hands the shared checks a pointer they accept in the boundary cells' place)
static inline const float *ring_or(MacroBoundary bound, const float *r, const float *ghost) { return bound == kBoundRing ? r : ghost; }
static int macro_rollout_fwd_jvp_entry(const dhts_macro_desc *d, int T, int n_dir,
                               const float *r, const float *y, const float *u, const float *ueq, const float *ghost, MacroBoundary bound,
                               const float *t_r, const float *t_y, const float *t_ghost,
                               float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                               const int32_t *det, int n_det, float *taps, float *t_taps,
                               dhts_error *err, dhts_error *err_jvp, void *stream,
                               const int32_t *ramps = nullptr, int n_ramp = 0, const float *inflow = nullptr, const float *t_inflow = nullptr) {
    if (!macro_fwd_args_ok(d, T, r, y, u, ueq, ring_or(bound, r, ghost), r_out, y_out, u_out, ueq_out) || n_dir < 1 || !t_r || !t_y ||
        !t_r_out || !t_y_out)
        return DHTS_E_INVALID;
    if (!macro_det_pair_ok(d, det, n_det, taps) || !macro_det_pair_ok(d, det, n_det, t_taps)) return DHTS_E_INVALID;
    // the ramp entry points: no ramp is the sibling's call; the arrays only where a step reads them (t_inflow NULL: zero tangents)
    if (n_ramp < 0 || (n_ramp > 0 && T > 0 && (!ramps || !inflow))) return DHTS_E_INVALID;
    if (macro_fwd_jvp_plan(d, T, n_dir).kmax < 1) return DHTS_E_INVALID;       // the lane does not fit: the taped pair covers it
    MacroTangents t = {t_r, t_y, t_ghost, t_r_out, t_y_out, t_taps, nullptr};
    if (T == 0) {                                                // no step: state and tangents come back as they went in, no row is addressed
        if (!macro_tangents_copy(d, n_dir, t, stream)) return DHTS_E_LAUNCH;
        return macro_state_copy(d, r, y, u, ueq, r_out, y_out, u_out, ueq_out, stream);
    }
    MacroForm f = macro_bound_form(bound, det, n_det);
    f.taps = taps;
    if (n_ramp > 0) { f.ramps = ramps; f.n_ramp = n_ramp; f.inflow = inflow; t.inflow = t_inflow; }
    return macro_fwd_jvp_launch(d, T, n_dir, r, y, u, ueq, ghost, t, r_out, y_out, u_out, ueq_out, f, err, err_jvp, stream);
}
int dhts_macro_rollout_fwd_jvp(const dhts_macro_desc *d, int T, int n_dir,
                               const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                               const float *t_r, const float *t_y, const float *t_ghost,
                               float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                               const int32_t *det, int n_det, float *taps, float *t_taps,
                               dhts_error *err, dhts_error *err_jvp, void *stream) {
    return macro_rollout_fwd_jvp_entry(d, T, n_dir, r, y, u, ueq, ghost, ghost_is_sched ? kBoundSched : kBoundConst, t_r, t_y, t_ghost, r_out,
                                       y_out, u_out, ueq_out, t_r_out, t_y_out, det, n_det, taps, t_taps, err, err_jvp, stream);
}
int dhts_macro_rollout_fwd_jvp_ring(const dhts_macro_desc *d, int T, int n_dir,
                                    const float *r, const float *y, const float *u, const float *ueq, const float *t_r, const float *t_y,
                                    float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                                    const int32_t *det, int n_det, float *taps, float *t_taps,
                                    dhts_error *err, dhts_error *err_jvp, void *stream) {
    return macro_rollout_fwd_jvp_entry(d, T, n_dir, r, y, u, ueq, nullptr, kBoundRing, t_r, t_y, nullptr, r_out, y_out, u_out, ueq_out,
                                       t_r_out, t_y_out, det, n_det, taps, t_taps, err, err_jvp, stream);
}
int dhts_macro_fwd_jvp_plan(const dhts_macro_desc *d, int T, int n_dir, int n_det, int32_t plan[8]) {
    if (!macro_desc_ok(d) || T < 0 || n_dir < 1 || !plan || n_det < 0 || n_det > d->n_cells) return DHTS_E_INVALID;
    const FwdJvpPlan pl = macro_fwd_jvp_plan(d, T, n_dir);
    plan[0] = pl.W; plan[1] = pl.p; plan[2] = pl.widest; plan[3] = pl.launches; plan[4] = (int32_t)pl.lds;
    plan[5] = plan[6] = plan[7] = 0;
    return DHTS_OK;
}
// ---- reverse mode from checkpoints, the segment's interface products in LDS ------------------------------------------------------
int dhts_macro_ckpt_plan(const dhts_macro_desc *d, int T, int n_det, int segment, int32_t plan[8]) {
    if (!macro_desc_ok(d) || T < 0 || !plan || n_det < 0 || n_det > d->n_cells || segment < 0) return DHTS_E_INVALID;
    return macro_ckpt_plan_fill(d, T, segment, false, plan);
}
size_t dhts_macro_ckpt_bytes(const dhts_macro_desc *d, int T, int segment) {
    if (!macro_desc_ok(d) || T < 0) return 0;
    const int S = macro_ckpt_segment(macro_ckpt_plan(d), segment);
    if (S < 0) return 0;
    return (size_t)macro_ckpt_count(T, S) * d->n_lanes * macro_ckpt_row_bytes(d->n_cells);
}
// The on-ramp arguments of the _ramp entry points (on: the call is one of them); the entry functions below serve both kinds.
struct MacroRamps {
    bool on;
    const int32_t *ramps;
    int n_ramp;
    const float *inflow;
    float *g_inflow;
};
// n_ramp in 1 .. n_cells whatever T is; the arrays only where a step reads or writes them.  d: checked by the caller
static inline bool macro_ramps_ok(const dhts_macro_desc *d, int T, const MacroRamps &ra, bool reverse) {
    if (!ra.on) return true;
    if (ra.n_ramp < 1 || ra.n_ramp > d->n_cells) return false;
    return T <= 0 || (ra.ramps && ra.inflow && (!reverse || ra.g_inflow));
}
static inline void macro_ramps_form(MacroForm &f, const MacroRamps &ra) {
    if (!ra.on) return;
    f.ramps = ra.ramps; f.n_ramp = ra.n_ramp; f.inflow = ra.inflow; f.g_inflow = ra.g_inflow;
}
// the reverse sweep's owner of a ramp cell writes that cell's column of g_inflow; a column whose index is outside [0, N) has no owner
// and keeps the zero it gets here
static inline bool macro_ramps_clear(const dhts_macro_desc *d, int T, const MacroRamps &ra, void *stream) {
    return !ra.on || hipMemsetAsync(ra.g_inflow, 0, sizeof(float) * (size_t)T * d->n_lanes * ra.n_ramp, (hipStream_t)stream) == hipSuccess;
}
static int macro_rollout_fwd_ckpt_entry(const dhts_macro_desc *d, int T, int segment,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, MacroBoundary bound,
                                float *r_out, float *y_out, float *u_out, float *ueq_out,
                                const int32_t *det, int n_det, float *taps, void *ckpt, dhts_error *err, void *stream,
                                const MacroRamps &ra = {}) {
    if (!macro_fwd_args_ok(d, T, r, y, u, ueq, ring_or(bound, r, ghost), r_out, y_out, u_out, ueq_out) || (T > 0 && !ckpt)) return DHTS_E_INVALID;
    if (!macro_det_pair_ok(d, det, n_det, taps) || !macro_ramps_ok(d, T, ra, false)) return DHTS_E_INVALID;
    const MacroCkptPlan pl = macro_ckpt_plan(d);
    const int S = macro_ckpt_segment(pl, segment);
    if (S < 0) return DHTS_E_INVALID;
    if (T == 0) return macro_state_copy(d, r, y, u, ueq, r_out, y_out, u_out, ueq_out, stream);
    MacroForm f = macro_bound_form(bound, det, n_det);
    f.taps = taps;
    macro_ramps_form(f, ra);
    return macro_ckpt_fwd_launch(d, T, S, pl, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out, ckpt, f, err, stream);
}
int dhts_macro_rollout_fwd_ckpt(const dhts_macro_desc *d, int T, int segment,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                float *r_out, float *y_out, float *u_out, float *ueq_out,
                                const int32_t *det, int n_det, float *taps, void *ckpt, dhts_error *err, void *stream) {
    return macro_rollout_fwd_ckpt_entry(d, T, segment, r, y, u, ueq, ghost, ghost_is_sched ? kBoundSched : kBoundConst, r_out, y_out, u_out,
                                        ueq_out, det, n_det, taps, ckpt, err, stream);
}
int dhts_macro_rollout_fwd_ckpt_ring(const dhts_macro_desc *d, int T, int segment,
                                     const float *r, const float *y, const float *u, const float *ueq,
                                     float *r_out, float *y_out, float *u_out, float *ueq_out,
                                     const int32_t *det, int n_det, float *taps, void *ckpt, dhts_error *err, void *stream) {
    return macro_rollout_fwd_ckpt_entry(d, T, segment, r, y, u, ueq, nullptr, kBoundRing, r_out, y_out, u_out, ueq_out, det, n_det, taps,
                                        ckpt, err, stream);
}
// what both checkpointed reverse entry points ask of the replay's inputs, the seeds and the outputs
static inline bool macro_replay_args_ok(const dhts_macro_desc *d, int T, const void *ckpt, const float *r, const float *y, const float *u,
                                        const float *ueq, const float *ghost, MacroBoundary bound, const float *g_r, const float *g_y,
                                        const float *g_r_out, const float *g_y_out, const double *g_ghost) {
    return macro_desc_ok(d) && T >= 0 && (T == 0 || ckpt) && r && y && u && ueq && ring_or(bound, r, ghost) && g_r && g_y && g_r_out &&
           g_y_out && (bound != kBoundSched || g_ghost);
}
static int macro_rollout_bwd_ckpt_entry(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, MacroBoundary bound,
                                const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream, const MacroRamps &ra = {}) {
    if (!macro_replay_args_ok(d, T, ckpt, r, y, u, ueq, ghost, bound, g_r, g_y, g_r_out, g_y_out, g_ghost)) return DHTS_E_INVALID;
    if (!macro_det_pair_ok(d, det, n_det, g_taps) || !macro_ramps_ok(d, T, ra, true)) return DHTS_E_INVALID;
    const MacroCkptPlan pl = macro_ckpt_plan(d);
    const int S = macro_ckpt_segment(pl, segment);
    if (S < 0) return DHTS_E_INVALID;
    if (T == 0) {        // no step: the cotangents come back as they went in, the boundary sums are zero, no row is addressed
        const size_t bytes = sizeof(float) * (size_t)d->n_lanes * d->n_cells;
        if (!macro_copy_back(g_r_out, g_r, bytes, stream) || !macro_copy_back(g_y_out, g_y, bytes, stream)) return DHTS_E_LAUNCH;
        if (bound == kBoundConst && g_ghost &&
            hipMemsetAsync(g_ghost, 0, sizeof(double) * 4 * (size_t)d->n_lanes, (hipStream_t)stream) != hipSuccess)
            return DHTS_E_LAUNCH;
        return DHTS_OK;
    }
    MacroForm f = macro_bound_form(bound, det, n_det);
    f.g_cot = g_taps;
    macro_ramps_form(f, ra);
    if (!macro_ramps_clear(d, T, ra, stream)) return DHTS_E_LAUNCH;
    return macro_ckpt_bwd_launch(d, T, S, pl, ckpt, r, y, u, ueq, ghost, g_r, g_y, g_r_out, g_y_out, g_ghost, f, err, stream);
}
int dhts_macro_rollout_bwd_ckpt(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                float *g_r_out, float *g_y_out, double *g_ghost, dhts_error *err, void *stream) {
    return macro_rollout_bwd_ckpt_entry(d, T, segment, ckpt, r, y, u, ueq, ghost, ghost_is_sched ? kBoundSched : kBoundConst, g_r, g_y, det,
                                        n_det, g_taps, g_r_out, g_y_out, g_ghost, err, stream);
}
int dhts_macro_rollout_bwd_ckpt_ring(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                     const float *r, const float *y, const float *u, const float *ueq,
                                     const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                     float *g_r_out, float *g_y_out, dhts_error *err, void *stream) {
    return macro_rollout_bwd_ckpt_entry(d, T, segment, ckpt, r, y, u, ueq, nullptr, kBoundRing, g_r, g_y, det, n_det, g_taps, g_r_out,
                                        g_y_out, nullptr, err, stream);
}
// ---- the dense-fit loss inside the checkpointed pair ----------------------------------------------------------------------------
int dhts_macro_ckpt_target_plan(const dhts_macro_desc *d, int T, int segment, int32_t plan[8]) {
    if (!macro_desc_ok(d) || T < 0 || !plan || segment < 0) return DHTS_E_INVALID;
    return macro_ckpt_plan_fill(d, T, segment, true, plan);
}
static int macro_rollout_fwd_ckpt_target_entry(const dhts_macro_desc *d, int T, int segment,
                                       const float *r, const float *y, const float *u, const float *ueq, const float *ghost, MacroBoundary bound,
                                       float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt, const float *target, double *sse,
                                       dhts_error *err, void *stream, const MacroRamps &ra = {}) {
    if (!macro_fwd_args_ok(d, T, r, y, u, ueq, ring_or(bound, r, ghost), r_out, y_out, u_out, ueq_out) || !sse || (T > 0 && !target) ||
        !macro_ramps_ok(d, T, ra, false))
        return DHTS_E_INVALID;
    const MacroCkptPlan pl = macro_ckpt_plan(d, true);
    const int S = macro_ckpt_segment(pl, segment);
    if (S < 0) return DHTS_E_INVALID;
    if (T == 0) {                                                // no step: no row is addressed, and the empty sums are 0
        if (hipMemsetAsync(sse, 0, sizeof(double) * 2 * (size_t)d->n_lanes, (hipStream_t)stream) != hipSuccess) return DHTS_E_LAUNCH;
        return macro_state_copy(d, r, y, u, ueq, r_out, y_out, u_out, ueq_out, stream);
    }
    MacroForm f = macro_bound_form(bound);
    f.target = target; f.sse = sse;
    macro_ramps_form(f, ra);
    return macro_ckpt_fwd_launch(d, T, S, pl, r, y, u, ueq, ghost, r_out, y_out, u_out, ueq_out, ckpt, f, err, stream);
}
int dhts_macro_rollout_fwd_ckpt_target(const dhts_macro_desc *d, int T, int segment,
                                       const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                       float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt, const float *target, double *sse,
                                       dhts_error *err, void *stream) {
    return macro_rollout_fwd_ckpt_target_entry(d, T, segment, r, y, u, ueq, ghost, ghost_is_sched ? kBoundSched : kBoundConst, r_out, y_out,
                                               u_out, ueq_out, ckpt, target, sse, err, stream);
}
int dhts_macro_rollout_fwd_ckpt_target_ring(const dhts_macro_desc *d, int T, int segment,
                                            const float *r, const float *y, const float *u, const float *ueq,
                                            float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt, const float *target,
                                            double *sse, dhts_error *err, void *stream) {
    return macro_rollout_fwd_ckpt_target_entry(d, T, segment, r, y, u, ueq, nullptr, kBoundRing, r_out, y_out, u_out, ueq_out, ckpt, target,
                                               sse, err, stream);
}
static int macro_rollout_bwd_ckpt_target_entry(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                       const float *r, const float *y, const float *u, const float *ueq, const float *ghost, MacroBoundary bound,
                                       const float *g_r, const float *g_y, const float *target, const double *g_sse, const float *r_fin,
                                       const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out, double *g_ghost,
                                       dhts_error *err, void *stream, const MacroRamps &ra = {}) {
    if (!macro_replay_args_ok(d, T, ckpt, r, y, u, ueq, ghost, bound, g_r, g_y, g_r_out, g_y_out, g_ghost) || !macro_ramps_ok(d, T, ra, true))
        return DHTS_E_INVALID;
    // the fit's cotangent needs the observations and the forward's final state (row T - 1 of the history)
    if (T > 0 && (!target || (g_sse && (!r_fin || !y_fin || !u_fin)))) return DHTS_E_INVALID;
    const MacroCkptPlan pl = macro_ckpt_plan(d, true);
    const int S = macro_ckpt_segment(pl, segment);
    if (S < 0) return DHTS_E_INVALID;
    if (T == 0 || !g_sse)            // no step, or no cotangent of the sums: the plain sweep (the segment is the TARGET plan's, which fits it)
        return macro_rollout_bwd_ckpt_entry(d, T, S, ckpt, r, y, u, ueq, ghost, bound, g_r, g_y, nullptr, 0, nullptr, g_r_out, g_y_out,
                                            g_ghost, err, stream, ra);
    MacroForm f = macro_bound_form(bound);
    f.target = target; f.g_sse = g_sse; f.fin_r = r_fin; f.fin_y = y_fin; f.fin_u = u_fin;
    macro_ramps_form(f, ra);
    if (!macro_ramps_clear(d, T, ra, stream)) return DHTS_E_LAUNCH;
    return macro_ckpt_bwd_launch(d, T, S, pl, ckpt, r, y, u, ueq, ghost, g_r, g_y, g_r_out, g_y_out, g_ghost, f, err, stream);
}
int dhts_macro_rollout_bwd_ckpt_target(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                       const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                       const float *g_r, const float *g_y, const float *target, const double *g_sse, const float *r_fin,
                                       const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out, double *g_ghost,
                                       dhts_error *err, void *stream) {
    return macro_rollout_bwd_ckpt_target_entry(d, T, segment, ckpt, r, y, u, ueq, ghost, ghost_is_sched ? kBoundSched : kBoundConst, g_r, g_y,
                                               target, g_sse, r_fin, y_fin, u_fin, g_r_out, g_y_out, g_ghost, err, stream);
}
int dhts_macro_rollout_bwd_ckpt_target_ring(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                            const float *r, const float *y, const float *u, const float *ueq,
                                            const float *g_r, const float *g_y, const float *target, const double *g_sse, const float *r_fin,
                                            const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out,
                                            dhts_error *err, void *stream) {
    return macro_rollout_bwd_ckpt_target_entry(d, T, segment, ckpt, r, y, u, ueq, nullptr, kBoundRing, g_r, g_y, target, g_sse, r_fin, y_fin,
                                               u_fin, g_r_out, g_y_out, nullptr, err, stream);
}
// ---- on-ramp inflow at chosen cells of the checkpointed pair -------------------------------------------------------
// ring != 0: a closed lane, which has no boundary cells (ghost must be NULL); else ghost is a schedule where ghost_is_sched
static inline bool macro_ramp_bound(int ring, const float *ghost, int ghost_is_sched, MacroBoundary &bound) {
    bound = ring ? kBoundRing : (ghost_is_sched ? kBoundSched : kBoundConst);
    return !ring || !ghost;
}
int dhts_macro_rollout_fwd_ckpt_ramp(const dhts_macro_desc *d, int T, int segment,
                                     const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                     float *r_out, float *y_out, float *u_out, float *ueq_out,
                                     const int32_t *det, int n_det, float *taps, void *ckpt,
                                     const int32_t *ramps, int n_ramp, const float *inflow, int ring, dhts_error *err, void *stream) {
    MacroBoundary bound;
    if (!macro_ramp_bound(ring, ghost, ghost_is_sched, bound)) return DHTS_E_INVALID;
    return macro_rollout_fwd_ckpt_entry(d, T, segment, r, y, u, ueq, ghost, bound, r_out, y_out, u_out, ueq_out, det, n_det, taps, ckpt, err,
                                        stream, MacroRamps{true, ramps, n_ramp, inflow, nullptr});
}
int dhts_macro_rollout_bwd_ckpt_ramp(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                     const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                     const float *g_r, const float *g_y, const int32_t *det, int n_det, const float *g_taps,
                                     float *g_r_out, float *g_y_out, double *g_ghost,
                                     const int32_t *ramps, int n_ramp, const float *inflow, float *g_inflow, int ring, dhts_error *err,
                                     void *stream) {
    MacroBoundary bound;
    if (!macro_ramp_bound(ring, ghost, ghost_is_sched, bound)) return DHTS_E_INVALID;
    return macro_rollout_bwd_ckpt_entry(d, T, segment, ckpt, r, y, u, ueq, ghost, bound, g_r, g_y, det, n_det, g_taps, g_r_out, g_y_out,
                                        ring ? nullptr : g_ghost, err, stream, MacroRamps{true, ramps, n_ramp, inflow, g_inflow});
}
int dhts_macro_rollout_fwd_ckpt_target_ramp(const dhts_macro_desc *d, int T, int segment,
                                            const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                            int ghost_is_sched, float *r_out, float *y_out, float *u_out, float *ueq_out, void *ckpt,
                                            const float *target, double *sse,
                                            const int32_t *ramps, int n_ramp, const float *inflow, int ring, dhts_error *err, void *stream) {
    MacroBoundary bound;
    if (!macro_ramp_bound(ring, ghost, ghost_is_sched, bound)) return DHTS_E_INVALID;
    return macro_rollout_fwd_ckpt_target_entry(d, T, segment, r, y, u, ueq, ghost, bound, r_out, y_out, u_out, ueq_out, ckpt, target, sse, err,
                                               stream, MacroRamps{true, ramps, n_ramp, inflow, nullptr});
}
int dhts_macro_rollout_bwd_ckpt_target_ramp(const dhts_macro_desc *d, int T, int segment, const void *ckpt,
                                            const float *r, const float *y, const float *u, const float *ueq, const float *ghost,
                                            int ghost_is_sched, const float *g_r, const float *g_y, const float *target, const double *g_sse,
                                            const float *r_fin, const float *y_fin, const float *u_fin, float *g_r_out, float *g_y_out,
                                            double *g_ghost, const int32_t *ramps, int n_ramp, const float *inflow, float *g_inflow, int ring,
                                            dhts_error *err, void *stream) {
    MacroBoundary bound;
    if (!macro_ramp_bound(ring, ghost, ghost_is_sched, bound)) return DHTS_E_INVALID;
    return macro_rollout_bwd_ckpt_target_entry(d, T, segment, ckpt, r, y, u, ueq, ghost, bound, g_r, g_y, target, g_sse, r_fin, y_fin, u_fin,
                                               g_r_out, g_y_out, ring ? nullptr : g_ghost, err, stream,
                                               MacroRamps{true, ramps, n_ramp, inflow, g_inflow});
}
// ---- on-ramp inflow and its tangent on the fused forward + tangent kernel -------------------------------------------
int dhts_macro_rollout_fwd_jvp_ramp(const dhts_macro_desc *d, int T, int n_dir,
                                    const float *r, const float *y, const float *u, const float *ueq, const float *ghost, int ghost_is_sched,
                                    const float *t_r, const float *t_y, const float *t_ghost,
                                    float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                                    const int32_t *det, int n_det, float *taps, float *t_taps,
                                    dhts_error *err, dhts_error *err_jvp, void *stream,
                                    const int32_t *ramps, int n_ramp, const float *inflow, const float *t_inflow) {
    return macro_rollout_fwd_jvp_entry(d, T, n_dir, r, y, u, ueq, ghost, ghost_is_sched ? kBoundSched : kBoundConst, t_r, t_y, t_ghost, r_out,
                                       y_out, u_out, ueq_out, t_r_out, t_y_out, det, n_det, taps, t_taps, err, err_jvp, stream, ramps, n_ramp,
                                       inflow, t_inflow);
}
int dhts_macro_rollout_fwd_jvp_ring_ramp(const dhts_macro_desc *d, int T, int n_dir,
                                         const float *r, const float *y, const float *u, const float *ueq, const float *t_r, const float *t_y,
                                         float *r_out, float *y_out, float *u_out, float *ueq_out, float *t_r_out, float *t_y_out,
                                         const int32_t *det, int n_det, float *taps, float *t_taps,
                                         dhts_error *err, dhts_error *err_jvp, void *stream,
                                         const int32_t *ramps, int n_ramp, const float *inflow, const float *t_inflow) {
    return macro_rollout_fwd_jvp_entry(d, T, n_dir, r, y, u, ueq, nullptr, kBoundRing, t_r, t_y, nullptr, r_out, y_out, u_out, ueq_out,
                                       t_r_out, t_y_out, det, n_det, taps, t_taps, err, err_jvp, stream, ramps, n_ramp, inflow, t_inflow);
}
int dhts_macro_state_from_ru_jvp(int64_t n, double u_max, const float *r, const float *u, const float *t_r, const float *t_u, float *t_y,
                                 void *stream) {
    if (n < 0 || !r || !u || !t_r || !t_u || !t_y) return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(macro_state_from_ru_jvp_kernel, grid_1d(n), 256, 0, stream, n, (float)u_max, r, u, t_r, t_u, t_y);
    return launch_status();
}
int dhts_macro_u_tap_jvp(int64_t n, double u_max, const float *r, const float *y, const float *t_r, const float *t_y, float *t_u,
                         void *stream) {
    if (n < 0 || !r || !y || !t_r || !t_y || !t_u) return DHTS_E_INVALID;
    if (n == 0) return DHTS_OK;
    launch(macro_u_tap_jvp_kernel, grid_1d(n), 256, 0, stream, n, (float)u_max, r, y, t_r, t_y, t_u);
    return launch_status();
}

}  // extern "C"
