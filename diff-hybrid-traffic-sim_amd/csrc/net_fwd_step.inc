// One step of net_macro_fwd_kernel (network_kernels.hip), included in that kernel's scope once per role set: kRole = 0 every
// role (no wavefronts of their own for the loss), 1 the physics threads' copy of the step loop, 2 the loss threads' copy.  Not a
// header of its own: it uses the kernel's local variables and lambdas by name.
        const float *cur = (t & 1) ? S1 : S0;
        float *nxt = (t & 1) ? S0 : S1;
        const int src = p_src, gate = p_gate; const double sched = p_sched;
        if (kRole != 2) fetch(t + 1);
        // ---- phase 1: ghosts of step t (_simulator.py:56-137) | loss scan of the state after step t-1
        if (kRole != 2 && is_ghost) {
            float fr, fu, fy, fq;
            if (g_side == 0) {
                // A source lane's ghost is Python floats in the reference (_simulator.py:68-71) and enters the solve as such: the lane's
                // first interface thread finds the doubles in ITS flux slots (written two barriers from now, read one barrier ago), a
                // NaN there says "an ordinary float32 ghost"
                double *fq0 = Fq + 2 * ((lfl[g_lane] & 0xffff) + g_lane);
                if (src < 0) {
                    const double gu = um_d * (1. - sqrt(fmax(sched, 0.) + kEps));
                    fr = (float)sched; fu = (float)gu; fy = 0.f; fq = (float)gu;      // y = r (u - u_eq(r)) = 0
                    fq0[0] = sched; fq0[1] = gu;
                } else {
                    fq0[0] = __longlong_as_double(0x7ff8000000000000ll);
                    const int last = lfl[src] >> 16;
                    const float gr = cur[last], gu = cur[2 * C + last];
                    float s = 1.f;
                    if (gate == -1) s = 0.f;
                    else if (gate >= 0) {
                        const int kd = linfo[gate] & 3;
                        if (kd != 0) s = sig[4 * (linfo[gate] >> 2) + (kd - 1)];
                    }
                    ghost_up_blend(gr, gu, s, um, fr, fu);
                    glue_from_r_u(fr, fu, um, fy, fq);
                }
            } else {
                float gr = own_r, gu = own_u;
                if (src >= 0) { const int first = lfl[src] & 0xffff; gr = cur[first]; gu = cur[2 * C + first]; }
                else if (!kHard) { own_w[(size_t)t * 2 * L + 2 * g_lane] = gr; own_w[(size_t)t * 2 * L + 2 * g_lane + 1] = gu; }
                const float sg = g_kind != 0 ? sig[4 * g_inter + (g_kind - 1)] : 1.f;
                const float s2 = kHard ? (sg > 0.5f ? 1.f : 0.f) : soft_switch(sg - 0.5f, kSigK);
                ghost_down_blend(gr, gu, s2, fr, fu);
                glue_from_r_u(fr, fu, um, fy, fq);
                own_r = fr; own_u = fu;
            }
            float *g = G + (size_t)(2 * g_lane + g_side) * 4;
            g[0] = fr; g[1] = fy; g[2] = fu; g[3] = fq;
        }
        NET_STAMP(0)
        if (kRole != 1 && t > 0) loss_scan(cur);
        NET_STAMP(1)
        lds_barrier();
        NET_STAMP(6)
        // ---- phase 2: interface solves | loss constants
        if (kRole != 2 && is_if) {
            const float *gl = G + (size_t)(2 * i_lane) * 4, *gr_ = G + (size_t)(2 * i_lane + 1) * 4;
            double rL, yL, uL, qL, rR, yR, uR, qR;
            if (i_k == 0) {
                const double sr = Fq[2 * tid];
                if (sr == sr) { rL = sr; yL = 0.; uL = Fq[2 * tid + 1]; qL = uL; }         // source lane: the ghost in double
                else { rL = gl[0]; yL = gl[1]; uL = gl[2]; qL = gl[3]; }
            }
            else { const int c = i_off + i_k - 1; rL = cur[c]; yL = cur[C + c]; uL = cur[2 * C + c]; qL = cur[3 * C + c]; }
            if (i_k == i_n) { rR = gr_[0]; yR = gr_[1]; uR = gr_[2]; qR = gr_[3]; }
            else { const int c = i_off + i_k; rR = cur[c]; yR = cur[C + c]; uR = cur[2 * C + c]; qR = cur[3 * C + c]; }
            Iface f;
            arz_interface(rL, yL, uL, qL, rR, yR, uR, qR, kconst, f);
            if (f.cfl_bad && fault_step < 0) { fault_step = t; fault_index = i_k; }
            Fq[2 * tid] = f.Fr; Fq[2 * tid + 1] = f.Fy;
            float *ab = AB + (size_t)tid * 8;
            ab[0] = f.A[0]; ab[1] = f.A[1]; ab[2] = f.A[2]; ab[3] = f.A[3];
            ab[4] = f.B[0]; ab[5] = f.B[1]; ab[6] = f.B[2]; ab[7] = f.B[3];
        }
        NET_STAMP(2)
        if (kRole != 1 && t > 0) loss_consts(cur, t - 1);
        NET_STAMP(3)
        lds_barrier();
        NET_STAMP(6)
        // ---- phase 3: cell updates + tape + history (_macro_lane.py:103-114, dmacro_lane.py:126-129) | lane queues
        if (kRole != 2 && is_cell) {
            const int c = tid;
            const float cf = (float)c_cc, ncf = (float)(-c_cc);
            const int iL = c + c_lane, iR = iL + 1;
            const float nr = (float)((double)cur[c] + (Fq[2 * iL] - Fq[2 * iR]) * c_cc);
            const float ny = (float)((double)cur[C + c] + (Fq[2 * iL + 1] - Fq[2 * iR + 1]) * c_cc);
            float nu, nq;
            glue_from_r_y(nr, ny, um, nu, nq);
            nxt[c] = nr; nxt[C + c] = ny; nxt[2 * C + c] = nu; nxt[3 * C + c] = nq;
            if (!kHard) {
                float *hn = hist_r + (size_t)(t + 1) * 4 * C;
                hn[c] = nr; hn[C + c] = ny; hn[2 * C + c] = nu; hn[3 * C + c] = nq;
                const float *aL = AB + (size_t)iL * 8, *aR = AB + (size_t)iR * 8;
                float4 d0, d1, d2;                      // cell_blocks (arz_device.hpp) restated on the floats of the AB slots
                d0.x = ncf * (-aL[0]); d0.y = ncf * (-aL[1]); d0.z = ncf * (-aL[2]); d0.w = ncf * (-aL[3]);
                d2.x = ncf * aR[4]; d2.y = ncf * aR[5]; d2.z = ncf * aR[6]; d2.w = ncf * aR[7];
                d1.x = 1.f - cf * (aR[0] - aL[4]); d1.y = 0.f - cf * (aR[1] - aL[5]);
                d1.z = 0.f - cf * (aR[2] - aL[6]); d1.w = 1.f - cf * (aR[3] - aL[7]);
                float4 *tp = tape_r + (size_t)t * 3 * Cp;
                tp[c] = d0; tp[Cp + c] = d1; tp[2 * Cp + c] = d2;
            }
        }
        NET_STAMP(4)
        if (kRole != 1 && t > 0) loss_lanes(t - 1);
        if (t + 1 < T) signals();            // of step t + 1 (this step's ghosts read theirs two barriers ago)
        NET_STAMP(5)
        lds_barrier();
        NET_STAMP(6)
    