// One step of net_hybrid_bwd_kernel (hybrid_kernels.hip), included twice in that kernel's scope: with kMw = true for the micro
// wave's copy of the step loop and with kMw = false for everybody else's (see the forward kernel).  Not a header of its own:
// it uses the kernel's local variables and lambdas by name.
        float *Hc = (t & 1) ? H1 : H0;           // row t
        const float *Hn = (t & 1) ? H0 : H1;     // row t+1
        // ================= R0: this step's data (fetched during the previous iteration) =================
        const float w_kc = p_kc; const float4 aL = p_aL, bL = p_bL, aR = p_aR, bR = p_bR;
        const unsigned w_capflag = p_capflag; const float2 w_capru = p_capru;
        const int src = p_src, gate = p_gate; const float w_own_r = p_own_r, w_own_u = p_own_u;
        if (!kMw && is_cell) { Hc[tid] = p_hr; Hc[C + tid] = p_hy; Hc[2 * C + tid] = p_hu; }
        // loss taps on the state after step t (row t + 1 is in LDS since the previous iteration): d reward / d q_l = -2 q_l dt
        // with q_l = sqrt(term / dt), evaluated by every cell for its own lane
        if (!kMw && is_cell && (!kState || gscale != 0.f)) {        // (a pure state tap passes g_reward = 0: the queue loss' constants are not even looked at)
            const int c = tid;
            const float gql = t < loss_steps ? gscale * (-1.0f) * (float)dt * 2.f * sqrtf(p_q / (float)dt) : 0.f;
            const float rr = Hn[c], uu = Hn[2 * C + c];
            const float x = s0f - uu;
            float sw, dsw;
            soft_switch_both(x, w_kc, sw, dsw);
            gL[c] += gql * sw * c_dxv;
            gL[2 * C + c] += gql * (rr * c_dxv) * (-dsw);
        }
        if (!kMw && is_sg) {
            float we, ns, a, pr; int ai;
            phase_signal_at(act, n_action, sq, F, rev_ph, rev_fr, sg_q, we, ns, a, pr, ai);
            sg[6 * sg_q] = we; sg[6 * sg_q + 1] = ns;
            signal_slopes(we, ns, a, pr, false, sg[6 * sg_q + 2], sg[6 * sg_q + 3]);
        }
        int seg_lo[kPhases], seg_n[kPhases];            // this lane's record segments of the step (micro wave)
#pragma unroll
        for (int ph = 0; ph < kPhases; ++ph) { seg_lo[ph] = 0; seg_n[ph] = 0; }
        if constexpr (kMw) {
            const int r_lo = p_rlo, n_rec = p_nrec;
            if (n_rec > tb.max_step_records) over = true;
            else {
#pragma unroll
                for (int j = 0; j < kPre; ++j) {
                    const int k = mw_lane + 64 * j;
                    if (k < n_rec) { rk[k] = p_rk[j]; *reinterpret_cast<int4 *>(ri + 4 * k) = p_ri[j]; *reinterpret_cast<float4 *>(rw + 4 * k) = p_rw[j]; }
                }
                for (int k = mw_lane + 64 * kPre; k < n_rec; k += 64) {
                    rk[k] = grk[r_lo + k];
                    *reinterpret_cast<int4 *>(ri + 4 * k) = gri[r_lo + k];
                    *reinterpret_cast<float4 *>(rw + 4 * k) = grw[r_lo + k];
                }
            }
            {   // a lane's block = its three segments back to back; blocks follow each other in lane order
                const int c = p_seg[0] + p_seg[1] + p_seg[2];
                const int inc = wave_scan_add(c);
                int lo_ = inc - c;
#pragma unroll
                for (int ph = 0; ph < kPhases; ++ph) { seg_lo[ph] = lo_; seg_n[ph] = over ? 0 : p_seg[ph]; lo_ += p_seg[ph]; }
            }
        }
        if constexpr (kMw) fetch_micro(t - 1); else fetch_cells(t - 1);
        HYB_BARRIER(0);
        // ================= R2: micro records of the loss / hand-off part, newest first =================
        bool used_ob = false;
        auto replay = [&](int lo_, int n_, int &n_sig) { // this lane's records [lo_, lo_ + n_), newest first (n_sig: signal records met so far)
            for (int k = lo_ + n_ - 1; k >= lo_; --k) {
                const int kw = rk[k];
                const int kind = kw >> 24, out = kw & 0xffffff;
                const int4 in4 = *reinterpret_cast<const int4 *>(ri + 4 * k);
                const float4 w4 = *reinterpret_cast<const float4 *>(rw + 4 * k);
                const int in[4] = {in4.x, in4.y, in4.z, in4.w};
                const float w[4] = {w4.x, w4.y, w4.z, w4.w};
                if (kind == K_NODE) {
                    const float a = adj[out];
                    adj[out] = 0.f;
                    if (a != 0.f) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) if (in[q] >= 0) adj[in[q]] += a * w[q];
                    }
                } else if (kind == K_IDM) {
                    const float gp = adj[out], gv = adj[out + 1];          // cotangents of the new (p, v)
                    float op = gp + w[0] * gv, ov = dtf * gp + w[1] * gv;   // dEgo^T
                    if (in[2]) {                                            // head: leader = (p + head_dp, v - head_dv)
                        op += w[2] * gv; ov += w[3] * gv;
                        if (in[0] >= 0) adj[in[0]] += w[2] * gv;
                        if (in[1] >= 0) adj[in[1]] -= w[3] * gv;
                    } else {
                        adj[in[0]] += w[2] * gv;
                        adj[in[1]] += w[3] * gv;
                    }
                    adj[out] = op; adj[out + 1] = ov;
                } else if (kind == K_COMMIT) {
                    if (in[0] >= 0) adj[in[0]] += adj[out];
                    adj[out] = 0.f;
                } else if (kind == K_SEED) {
                    if (!kState || gscale != 0.f) adj[in[0]] += gscale * w[0];
                } else if (kind == K_DEPOSIT) {
                    const int c = in[3];
                    const float n_r = w[2], speed = Hn[2 * C + c];
                    float g_nr = gL[c], g_speed = gL[2 * C + c];
                    glue_y_bwd(n_r, speed, um, gL[C + c], g_nr, g_speed);
                    const float dx = (float)tb.net.lane_dx[out];
                    if (in[0] >= 0) adj[in[0]] += g_nr * ((w[0] / dx) / vlen);
                    if (in[1] >= 0) adj[in[1]] += g_nr * ((w[3] / vlen) / dx) * w[1];
                    if (in[2] >= 0) adj[in[2]] += g_speed;
                    gL[c] = g_nr; gL[C + c] = 0.f; gL[2 * C + c] = 0.f;
                } else if (kind == K_CELLREAD) {
                    gL[in[2]] += adj[in[0]];
                    gL[2 * C + in[2]] += adj[in[1]];
                    adj[in[0]] = 0.f; adj[in[1]] = 0.f;
                } else if (kind == K_SIGNAL) {
                    // several lanes may look at the same intersection: through the outbox, applied in lane order
                    used_ob = true;
                    if (n_sig < 3) { obi[mw_lane * 5 + 2 + n_sig] = in[1]; obf[mw_lane * 5 + 2 + n_sig] = adj[in[0]] * sg[6 * in[1] + 2 + (in[2] - 1)]; }
                    ++n_sig;
                    adj[in[0]] = 0.f;
                } else if (kind == K_IMPORT) {
                    // the leader's position / speed slots belong to another lane
                    used_ob = true;
                    obi[mw_lane * 5 + 0] = in[2]; obf[mw_lane * 5 + 0] = adj[in[0]];
                    obi[mw_lane * 5 + 1] = in[3]; obf[mw_lane * 5 + 1] = adj[in[1]];
                    adj[in[0]] = 0.f; adj[in[1]] = 0.f;
                }
            }
        };
        if constexpr (kMw) {
            int n_sig2 = 0, n_sig1 = 0;                  // (signal records only occur in the first segment)
            replay(seg_lo[2], seg_n[2], n_sig2);         // the vehicles' loss terms, then the commits
            // A capacitor's charge precedes ALL hand-off events of its step (a deposit may rewrite the very cell it read), and
            // lanes replay side by side: the events of every lane first (lane 0 holds them), the capacitors afterwards
            replay(seg_lo[1], seg_n[1], n_sig1);
            // cap' = cap + (r u) dt (no record since round 3): the slot's cotangent passes through to the previous level if that
            // was a variable and reaches the cell as ((a dt) u, (a dt) r); the u leaf may also carry a spawned vehicle's speed
            if (mw_lane < kMaxCaps && ((w_capflag >> mw_lane) & 1u)) {
                const int out = 3 * V + mw_lane, leaf = 3 * V + kMaxCaps + mw_lane;
                const float a = adj[out];
                adj[out] = ((w_capflag >> (16 + mw_lane)) & 1u) ? a : 0.f;
                const float ad = a * dtf;
                const float g_u = adj[leaf] + ad * w_capru.y;
                adj[leaf] = 0.f;
                gL[cap_last_r] += ad * w_capru.x;
                gL[2 * C + cap_last_r] += g_u;
            }
        }
        // ghost threads: the forward blend of this step's ghost (everything that needs no cotangent), while only the micro
        // wave has work; the cotangent part follows two phases later (ghost_up_bwd / ghost_down_bwd of net_device.hpp, cut in two here)
        float gh_gr = 0.f, gh_gu = 0.f, gh_s = 1.f, gh_fr = 0.f, gh_fu = 0.f, gh_ds = 0.f, gh_ds2 = 0.f; int gh_cell = -1, gh_kd = 0;
        if (!kMw && is_ghost && g_macro) {
            if (g_side == 0) {
                if (src >= 0) {
                    gh_cell = lfl[src] >> 16;
                    gh_gr = Hc[gh_cell]; gh_gu = Hc[2 * C + gh_cell];
                    int it = 0;
                    if (plain) gh_s = 1.f;               // (the neighbour's edge cell as it is: 1 * g + 0 * red below is exact)
                    else if (gate == -1) gh_s = 0.f;
                    else if (gate >= 0) { gh_kd = linfo[gate] & 3; it = linfo[gate] >> 2; if (gh_kd != 0) gh_s = sg[6 * it + (gh_kd - 1)]; }
                    ghost_up_blend(gh_gr, gh_gu, gh_s, um, gh_fr, gh_fu);
                    if (gh_kd != 0) gh_ds = sg[6 * it + 2 + (gh_kd - 1)];
                    if (gh_kd != 0 && it != g_inter) bad_key = true;
                }
            } else {
                gh_cell = src < 0 ? -1 : (lfl[src] & 0xffff);
                gh_gr = src < 0 ? w_own_r : Hc[gh_cell];
                gh_gu = src < 0 ? w_own_u : Hc[2 * C + gh_cell];
                const float sgl = g_kind != 0 ? sg[6 * g_inter + (g_kind - 1)] : 1.f;
                gh_s = plain ? 1.f : soft_switch(sgl - 0.5f, kSigK);
                ghost_down_blend(gh_gr, gh_gu, gh_s, gh_fr, gh_fu);
                if (g_kind != 0) { gh_ds = soft_switch_grad(sgl - 0.5f, kSigK); gh_ds2 = sg[6 * g_inter + 2 + (g_kind - 1)]; }
            }
        }
        HYB_BARRIER(1);
        // ================= R3: speed cotangents into (r, y); J^T g per cell =================
        float v_r = 0.f, v_y = 0.f;
        if (!kMw && is_cell) {
            const int c = tid;
            float gr = gL[c], gy = gL[C + c];
            glue_u_bwd(Hn[c], Hn[C + c], um, gL[2 * C + c], gr, gy);
            float4 d0, d1, d2;
            cell_blocks(aL, bL, aR, bR, c_cf, c_ncf, d0, d1, d2);
            c0[c] = dot2(d0.x, gr, d0.z, gy); c0[C + c] = dot2(d0.y, gr, d0.w, gy);
            c2[c] = dot2(d2.x, gr, d2.z, gy); c2[C + c] = dot2(d2.y, gr, d2.w, gy);
            v_r = dot2(d1.x, gr, d1.z, gy); v_y = dot2(d1.y, gr, d1.w, gy);
        }
        // micro wave: the step's first segment (IDM steps, then head gaps) touches the vehicles' cotangents and the outboxes only;
        // it is replayed in three parts beside the cells' last three phases (its newest third here), so that none of them waits
        // for this wave: what the outboxes hand to the intersections is taken by their rows one step later (gam, two buffers)
        int n_sig0 = 0, n_first0 = 0, n_second0 = 0;
        if constexpr (kMw) {
            // (a lane has a handful of records: thirds rounded towards the earlier phases measured best, 2.11 ms against 2.13-2.24
            // for other splits; R5 also applies the outboxes)
            n_first0 = (seg_n[0] + 2) / 3; n_second0 = (seg_n[0] - n_first0 + 1) >> 1;
            if (seg_n[0] > 0) for (int q = 0; q < 5; ++q) obi[mw_lane * 5 + q] = -1;
            replay(seg_lo[0] + (seg_n[0] - n_first0), n_first0, n_sig0);
        }
        HYB_BARRIER(2);
        // ================= R4: gather inside the lane; ghost cotangents | rest of the micro records =================
        if (!kMw && is_cell) {
            const int c = tid;
            if (c > c_first) { v_r += c2[c - 1]; v_y += c2[C + c - 1]; }
            if (c < c_last) { v_r += c0[c + 1]; v_y += c0[C + c + 1]; }
        }
        if (!kMw && is_ghost && g_macro) {
            float tgt = -1.f, add_r = 0.f, add_u = 0.f, a_val = 0.f;
            if (g_side == 0) {
                if (src >= 0) {
                    float g_fr = c0[g_off], g_fu = 0.f;
                    glue_y_bwd(gh_fr, gh_fu, um, c0[C + g_off], g_fr, g_fu);
                    add_r = g_fr * gh_s; add_u = g_fu * gh_s;
                    tgt = (float)gh_cell;
                    if (gh_kd != 0) a_val = ghost_up_switch_bwd(g_fr, g_fu, gh_gr, gh_gu, um) * gh_ds;
                }
            } else {
                const int lastc = g_off + g_n - 1;
                float g_fr = c2[lastc] + gown_r, g_fu = gown_u;      // the blended ghost is also the stored one
                glue_y_bwd(gh_fr, gh_fu, um, c2[C + lastc], g_fr, g_fu);
                if (src >= 0) { add_r = g_fr * gh_s; add_u = g_fu * gh_s; tgt = (float)gh_cell; gown_r = 0.f; gown_u = 0.f; }
                else { gown_r = g_fr * gh_s; gown_u = g_fu * gh_s; }
                if (g_kind != 0) {
                    a_val = ghost_down_switch_bwd(g_fr, g_fu, gh_gr, gh_gu) * gh_ds * gh_ds2;
                }
            }
            if (tgt >= 0.f) {
                float *box = g_side == 0 ? inL : inF;
#pragma unroll
                for (int i = 0; i < kMaxCand; ++i)
                    if (cand_src[i] == src) { box[3 * cand_pos[i]] = add_r; box[3 * cand_pos[i] + 1] = 0.f; box[3 * cand_pos[i] + 2] = add_u; }
            }
            aval[2 * g_lane + g_side] = a_val;          // the intersections sum their ghosts in (lane, side) order
        }
        if constexpr (kMw) replay(seg_lo[0] + (seg_n[0] - n_first0 - n_second0), n_second0, n_sig0);      // the middle part
        HYB_BARRIER(3);
        if constexpr (kMw) {
            replay(seg_lo[0], seg_n[0] - n_first0 - n_second0, n_sig0);      // the oldest part: the rest of the IDM steps, the head gaps
            unsigned long long obm = __ballot(used_ob);
            if (is_mt) {                                 // outboxes in lane order
                float *gam_w = gam + (t & 1) * sq;
                while (obm) {
                    const int s_ = __ffsll((long long)obm) - 1;
                    obm &= obm - 1;
                    for (int q = 0; q < 2; ++q) if (obi[s_ * 5 + q] >= 0) adj[obi[s_ * 5 + q]] += obf[s_ * 5 + q];
                    for (int q = 2; q < 5; ++q) if (obi[s_ * 5 + q] >= 0) gam_w[obi[s_ * 5 + q]] += obf[s_ * 5 + q];
                }
            }
        }
        // ================= R5: edge cells take their inboxes; action partials =================
        if (!kMw && is_cell) {
            float v_u = 0.f;
#pragma unroll
            for (int i = 0; i < kMaxEnt; ++i) {
                if (ent[i] >= 0) {
                    float *box = (ent[i] & 1) ? inF : inL;
                    const int k = ent[i] >> 1;
                    v_r += box[3 * k]; v_y += box[3 * k + 1]; v_u += box[3 * k + 2];
                    box[3 * k] = 0.f; box[3 * k + 1] = 0.f; box[3 * k + 2] = 0.f;
                }
            }
            gL[tid] = v_r; gL[C + tid] = v_y; gL[2 * C + tid] = v_u;
            if (bad_step < 0 && !(isfinite(v_r) && isfinite(v_y) && isfinite(v_u))) bad_step = t;
        }
        if (!kMw && in_rows) {
            double v = 0.;
            if (row_mode) {
                for (int k = iptr[own_q] + ((tid - row_base) & 15); k < iptr[own_q + 1]; k += 16) v += (double)aval[iidx[k]];
                v = row_scan_add(v);
            } else {
                for (int k = iptr[own_q]; k < iptr[own_q + 1]; ++k) v += (double)aval[iidx[k]];
            }
            if (is_own) {
                // what the micro wave's outboxes left for this intersection in step t + 1 (applied one phase late, in the other
                // buffer): it belongs to that step's phase, the one `ga` is still summing
                float *gam_r = gam + ((t + 1) & 1) * sq;
                ga += (double)gam_r[own_q]; gam_r[own_q] = 0.f;
                const int lastp = n_action / sq - 1;
                const int phase = rev_ph > lastp ? lastp : rev_ph;
                if (phase != cur_phase) { if (cur_phase >= 0) g_action[(size_t)rep * n_action + cur_phase * sq + own_q] = (float)ga; ga = 0.; cur_phase = phase; }
                ga += v;
            }
        }
        if (rev_fr == 0) { rev_fr = F - 1; --rev_ph; } else --rev_fr;
        HYB_BARRIER(4);
    