// Body of the per-graph forward, included into qnet_fwd_kernel and qnet_step_kernel (qnet_fused_kernels.h).  In scope: the
// arguments `a`, NT, MATH, JOBS and the macros QSEL / QMODE.  Kept as text, not as a function: a function called from two
// kernels, even force-inlined, changes the register allocation and the schedule of the existing instantiations.
    static_assert(!JOBS || MATH == 0, "the job-table form is exact fp32 only");
    using LD = QLds<NT>;
    constexpr int HP = LD::HP, XS = LD::XS, kHalf = LD::kHalf;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    f32x4* wbuf = reinterpret_cast<f32x4*>(lds + LD::off_w);       // [2][kHalf]
    float* xbuf = reinterpret_cast<float*>(lds + LD::off_x);       // [kRows][XS]
    const unsigned short* s_rp = reinterpret_cast<const unsigned short*>(lds + LD::off_rp);
    const unsigned char* s_col = reinterpret_cast<const unsigned char*>(lds + LD::off_col);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int job = [&] { if constexpr (JOBS) return __builtin_amdgcn_readfirstlane(a.jobs[blockIdx.x]); else return 0; }();
    const int gi = JOBS ? job >> 2 : (int)blockIdx.x, wset = JOBS ? job & (kMaxSets - 1) : 0;
    (void)wset;
    QSTAMP(0, 0, 0);
    // Requested before anything that depends on the graph (round 4): W_r of the first hidden layer (half B) and the raw first
    // layer's weights -- their round trips overlap the chain gptr -> rowptr -> columns instead of following it.
    constexpr int kStage1 = (LD::kHalf + 511) / 512, kStage0 = (2 * HP * kSmallCin / 4 + 511) / 512;
    f32x4 wstg1[kStage1], wstg0[kStage0];
    {
        const f32x4* src1 = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.fwd_off[a.L > 1 ? 1 : 0]) + kHalf;
#pragma unroll
        for (int k = 0; k < kStage1; ++k) { const int i = tid + 512 * k; if (a.L > 1 && i < kHalf) wstg1[k] = src1[i]; }
        const f32x4* src0 = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.fwd_off[0]);
#pragma unroll
        for (int k = 0; k < kStage0; ++k) { const int i = tid + 512 * k; if (i < 2 * HP * kSmallCin / 4) wstg0[k] = src0[i]; }
    }
    const int r0 = a.gptr[gi], r1 = a.gptr[gi + 1];
    const int cnt = r1 - r0;
    if (cnt > kRows) {
        // a graph that does not fit the tile reached this kernel (stale size hint): flag it AND poison its outputs, so
        // the failure is visible in the data even if nobody reads the status word
        if (tid == 0) {
            atomicOr(QSEL(status), 2);
            if constexpr (!JOBS) {
                if (a.out_v) a.out_v[gi] = __builtin_nanf("");
                if (a.td_sel && a.mode == 0) { a.td_out[gi] = __builtin_nanf(""); a.td_loss_part[gi] = __builtin_nanf(""); }
            }
        }
        for (int i = tid; i < cnt; i += 512) {
            QSEL(q)[r0 + i] = __builtin_nanf("");
            if constexpr (!JOBS) { if (a.td_sel && a.mode == 0) a.td_dq[r0 + i] = __builtin_nanf(""); }
        }
        return;
    }
    const int H = a.H;
    const int lrow = wave * 16 + r;                 // local row of this lane
    const bool rvalid = lrow < cnt;
    const bool wactive = wave * 16 < cnt;           // wave-uniform
    const bool spare = cnt <= kRows / 2;            // workgroup-uniform: waves 4-7 own no rows (dma_share)
    const int grow = r0 + lrow;
    // values the prologue needs two or three barriers further down are requested NOW, with the CSR: every global round trip
    // left on the chain gptr -> rowptr -> columns -> ... costs ~0.8 us at kernel start (GNN-S: 12.5 k ticks of prologue)
    const float idg = rvalid ? a.invdeg[grow] : 0.f;                 // hidden layers: 1 / deg of this lane's row
    const float sc0 = tid < cnt ? a.invdeg[r0 + tid] : 0.f;          // raw first layer: thread tid sums row tid
    // (the first layer's bias row too, at the narrow widths: at 97..112 columns its 28 registers cost the layer loop's
    // allocation 1.4 us, measured, and the bias is then read where it is used)
    constexpr bool kBiasAhead = NT <= 4;
    f32x4 b0v[kBiasAhead ? NT : 1];
    if constexpr (kBiasAhead) {
        const f32x4* b0 = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.bias_off[0]);
#pragma unroll
        for (int t = 0; t < NT; ++t) b0v[t] = b0[4 * t + g];
    }
    // (exact fp32: the first hidden layer's bias row, which its accumulators start from)
    f32x4 b1stg = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (MATH == 0) { if (a.L > 1 && tid < HP / 4) b1stg = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.bias_off[1])[tid]; }
    const int e0 = a.rowptr[r0], ne = a.rowptr[r1] - e0;
    const bool csr_lds = load_csr<NT>(lds, a.rowptr, a.col, r0, cnt, e0, ne, QSEL(status));
    float* s_max = reinterpret_cast<float*>(lds + LD::off_max);      // per-wave maxima (math 1)
    if (tid < 16) s_max[tid] = 0.f;
    if (tid < XS) xbuf[kRows * XS + tid] = 0.f;                      // the gather's filler row

    // ---- stage W_r of layer 1 into half B (the self half runs first); first-layer scratch lives in half A ----
    if (a.L > 1) {
#pragma unroll
        for (int k = 0; k < kStage1; ++k) { const int i = tid + 512 * k; if (i < kHalf) wbuf[kHalf + i] = wstg1[k]; }
    }
    NbrRegs nbr;
    float* s_w0 = reinterpret_cast<float*>(lds + LD::off_scr_first);  // [2][HP][8]
    float* s_f = s_w0 + 2 * HP * kSmallCin;                          // [kRows][16]: agg0 | x0
    {
        // raw features of the graph's rows -> LDS (x0 half of s_f), first-layer weights -> LDS: all independent
        // global loads, one barrier; the neighbour sums then run on LDS only.
#pragma unroll
        for (int k = 0; k < kStage0; ++k) {
            const int i = tid + 512 * k;
            if (i < 2 * HP * kSmallCin / 4) reinterpret_cast<f32x4*>(s_w0)[i] = wstg0[k];
        }
#pragma unroll
        for (int i = tid; i < kRows * kSmallCin; i += 512) {
            const int rr = i / kSmallCin, qq = i % kSmallCin;
            s_f[rr * 16 + 8 + qq] = (rr < cnt && qq < a.c_in) ? a.x[(size_t)(r0 + rr) * a.x_stride + qq] : 0.f;
        }
        __syncthreads();
        nbr = csr_lds ? load_nbrs<XS>(s_rp, s_col, lrow, rvalid, g)
                      : load_nbrs_global<XS>(a.rowptr, a.col, r0, cnt, e0, lrow, rvalid, g);
        if (tid < kRows) {
            float ag0[kSmallCin];
#pragma unroll
            for (int qq = 0; qq < kSmallCin; ++qq) ag0[qq] = 0.f;
            if (tid < cnt) {
                const int row = r0 + tid;
                if (csr_lds) {
                    for (int e = s_rp[tid]; e < s_rp[tid + 1]; ++e) {
                        const float* xr = s_f + (int)s_col[e] * 16 + 8;
#pragma unroll
                        for (int qq = 0; qq < kSmallCin; ++qq) ag0[qq] += xr[qq];
                    }
                } else {
                    for (int e = a.rowptr[row]; e < a.rowptr[row + 1]; ++e) {
                        const float* xr = s_f + (a.col[e] - r0) * 16 + 8;
#pragma unroll
                        for (int qq = 0; qq < kSmallCin; ++qq) ag0[qq] += xr[qq];
                    }
                }
#pragma unroll
                for (int qq = 0; qq < kSmallCin; ++qq) ag0[qq] *= sc0;
                if (!JOBS && a.need_backward) {
                    f32x4* ao = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.saved + a.agg_off[0]) + (size_t)row * kSmallCin);
                    ao[0] = f32x4{ag0[0], ag0[1], ag0[2], ag0[3]};
                    ao[1] = f32x4{ag0[4], ag0[5], ag0[6], ag0[7]};
                }
            }
#pragma unroll
            for (int qq = 0; qq < kSmallCin; ++qq) s_f[tid * 16 + qq] = ag0[qq];
        }
    }
    __syncthreads();

    // ---- layer 0 (raw features): every lane produces its own row chunks, already in the chained layout ----
    f32x4 xs[NT];
    {
        float f[16];
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) f[qq] = s_f[lrow * 16 + qq];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            f32x4 v;
            if constexpr (kBiasAhead) v = b0v[t];
            else v = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.bias_off[0])[4 * t + g];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int o = 16 * t + 4 * g + q4;
                const float* wl0 = s_w0 + o * kSmallCin;
                const float* wr0 = s_w0 + HP * kSmallCin + o * kSmallCin;
                float s = v[q4];
                if (a.c_in <= 2) {   // the model's raw features [degree, is_terminal]: the remaining packed weights are zero
                    s += wl0[0] * f[0] + wr0[0] * f[8];
                    s += wl0[1] * f[1] + wr0[1] * f[9];
                } else {
#pragma unroll
                    for (int qq = 0; qq < kSmallCin; ++qq) s += wl0[qq] * f[qq] + wr0[qq] * f[8 + qq];
                }
                v[q4] = rvalid ? fmaxf(s, 0.f) : 0.f;
            }
            xs[t] = v;
        }
        f32x4* xr = reinterpret_cast<f32x4*>(xbuf + lrow * XS) + g;
#pragma unroll
        for (int t = 0; t < NT; ++t) xr[4 * t] = xs[t];
        // (layer 0's rows go to global memory with the first hidden layer's fillers, like every other layer's: a store
        // here would be waited for at the barrier below)
    }
    if constexpr (MATH == 0) { if (tid < HP / 4) reinterpret_cast<f32x4*>(lds + LD::off_bias)[tid] = b1stg; }
    __syncthreads();   // xbuf + half B (+ the first hidden layer's bias row) visible; half A (scratch) free

    // ---- hidden layers ----
    const size_t slab = (size_t)a.n * HP;
    const float validf = rvalid ? 1.f : 0.f;
    QSTAMP(0, 0, 1);
    // Per layer two phases, each a K-half contraction that carries the layer's other work as fillers between its MFMAs:
    //   phase S: self half (W_r, half B) on the rows kept in registers; fillers = the LDS gather of the aggregate, the
    //            previous layer's saved-activation stores, LDS-DMA of W_l(l) into half A           -> barrier 1
    //   phase A: aggregate half (W_l, half A); fillers = the aggregate's saved-tensor stores, LDS-DMA of W_r(l+1) into
    //            half B; then bias + ReLU + new rows to LDS                                        -> barrier 2
    constexpr int kGaps = Gaps<NT, MATH>::value;
    constexpr int kDma = (NT * NT + 7) / 8;                  // LDS-DMA pieces per wave and half
    constexpr int kFill = kDma + NT;                         // filler slots used per phase
    constexpr int kTail = kFill > kGaps ? kGaps : kFill;     // narrow widths: the slots past the last gap run after the MFMAs
    float* s_bias = reinterpret_cast<float*>(lds + LD::off_bias);
    // where this lane's accumulators start (exact fp32): the bias row, or the all-zero row for a pad row
    const f32x4* binit = reinterpret_cast<const f32x4*>(rvalid ? s_bias : xbuf + kRows * XS) + g;
    const unsigned lds_w = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(lds + LD::off_w);
    const unsigned rowoff = (unsigned)grow * (HP * 4) + 16 * g;      // byte offset of this lane's slot inside a [n][HP] slab
    const unsigned lane16 = 16 * lane;
    auto acts_off = [&](const int l) -> unsigned {        // lane offset for storing layer l's rows (kOob: not stored)
        return (rvalid && (a.need_backward || a.acts_layer < 0 || a.acts_layer == l)) ? rowoff : kOob;
    };
    auto publish_xmax = [&](const int l) {   // layer maximum of [agg | x] over this graph -> global (order-independent);
        if constexpr (MATH == 1) {           // called one barrier after the waves wrote s_max
            if (a.xmax && tid == 0) {
                float mm = 0.f;
#pragma unroll
                for (int w8 = 0; w8 < 8; ++w8) mm = fmaxf(mm, s_max[w8]);
                atomicMax(a.xmax + l, __builtin_bit_cast(unsigned, mm));
            }
        }
    };
    for (int l = 1; l < a.L; ++l) {
        QSTAMP(0, l, 0);
        if (l > 1) publish_xmax(l - 1);
        const f32x4* wsrc = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.fwd_off[l]);
        const bool more = l + 1 < a.L;
        const f32x4* nsrc = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.fwd_off[more ? l + 1 : l]) + kHalf;
        // exact fp32: the NEXT layer's bias row is staged (its accumulators start from it); split math: this layer's
        f32x4 bstg = f32x4{0.f, 0.f, 0.f, 0.f};
        if (tid < HP / 4) bstg = reinterpret_cast<const f32x4*>(QSEL(wpack) + a.bias_off[(MATH == 0 && more) ? l + 1 : l])[tid];
        auto dmaS = [&](auto qq) {
            const int p = dma_share<NT>(wave, decltype(qq)::value, spare);
            if (p >= 0) dma_piece(wsrc + p * 64, lane16, lds_w + p * 1024);
            const int p2 = dma_share2<NT>(wave, decltype(qq)::value, spare);
            if (p2 >= 0) dma_piece(wsrc + p2 * 64, lane16, lds_w + p2 * 1024);
        };
        auto dmaA = [&](auto qq) {
            const int p = dma_share<NT>(wave, decltype(qq)::value, spare);
            if (more && p >= 0) dma_piece(nsrc + p * 64, lane16, lds_w + (kHalf + p * 64) * 16);
            const int p2 = dma_share2<NT>(wave, decltype(qq)::value, spare);
            if (more && p2 >= 0) dma_piece(nsrc + p2 * 64, lane16, lds_w + (kHalf + p2 * 64) * 16);
        };
        if (!wactive) {
            // a wave without rows only moves its weight pieces (its own straight path: the active path below then has no
            // `if (wactive)` regions whose merges cost register copies -- VALU instructions are MFMA time here)
            static_for<0, kDma>(dmaS);
            wait_vmem();
            if constexpr (MATH == 1) { if (tid < HP / 4) reinterpret_cast<f32x4*>(s_bias)[tid] = bstg; }
            lds_barrier();
            if constexpr (MATH == 0) { if (tid < HP / 4) reinterpret_cast<f32x4*>(s_bias)[tid] = bstg; }
            static_for<0, kDma>(dmaA);
            wait_vmem();
            lds_barrier();
            continue;
        }
        f32x4 acc[NT], ag[NT];
        if constexpr (MATH == 0) {
            // the accumulators start from the bias row (an LDS read instead of 14 zero moves + 14 adds in the epilogue);
            // pad rows start from the all-zero row and stay exactly zero through the ReLU
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = binit[4 * t];
        } else {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float rs = 1.f, rinv = 1.f, mx = 0.f;
        f32x4 tb[GatherLand<NT, MATH>::value][NT];
        if constexpr (MATH == 1) { mx = row_max4(frag_absmax<NT>(xs, 0.f)); row_scale(mx, rs, rinv); }
        // ---- phase S ----
        const __amdgpu_buffer_rsrc_t yprev = slab_rsrc(a.acts + slab * (l - 1));
        const unsigned yprev_off = acts_off(l - 1);
        auto fillS = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
            gather_gap<NT, Q, kGaps, MATH>(xbuf, nbr, ag, tb);
            if constexpr (Q < kDma) dmaS(qq);
            else if constexpr (Q < kDma + NT && !JOBS) buf_store(xs[Q - kDma], yprev, yprev_off + 64 * (Q - kDma));
        };
        contract_half_fill<NT, MATH>(wbuf + kHalf, lane, xs, acc, rs, fillS);
        static_for<kTail, kFill>(fillS);
        if (nbr.wlong) {      // (wave-uniform; pad rows: eb == ee)
            if (csr_lds) gather_lds<NT, XS>(xbuf, s_col, nbr.eb, nbr.ee, g, ag);
            else gather_global_tail<NT, XS>(xbuf, a.col, r0, cnt, e0 + nbr.eb, e0 + nbr.ee, g, ag);
        }
#pragma unroll
        for (int c = 0; c < NT; ++c) ag[c] *= idg;          // idg == 0 on pad rows
        QSTAMP(0, l, 1);
        wait_vmem();
        if constexpr (MATH == 1) { if (tid < HP / 4) reinterpret_cast<f32x4*>(s_bias)[tid] = bstg; }
        QSTAMP(0, l, 3);
        lds_barrier();     // barrier 1: half A = W_l(l) (+ bias row, split math); every gather of this layer is done; half B is free
        // (exact fp32: every wave has read this layer's bias row into its accumulators by now: the next layer's may land)
        if constexpr (MATH == 0) { if (tid < HP / 4) reinterpret_cast<f32x4*>(s_bias)[tid] = bstg; }
        QSTAMP(0, l, 4);
        // ---- phase A ----
        float rsa = 1.f;
        if constexpr (MATH == 1) {
            // the aggregate gets its own power-of-two row scale (it was not known when the self half ran); the self
            // half's sums are carried over by the exact ratio of the two scales
            float ma = row_max4(frag_absmax<NT>(ag, 0.f));
            if (a.xmax) { const float wm = rows_max16(fmaxf(ma, mx)); if (lane == 0) s_max[wave] = wm; }
            ma = fmaxf(ma, mx * 0x1p-40f);
            float rinva;
            row_scale(ma, rsa, rinva);
            const float carry = rsa * rinv;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] *= carry;
            rinv = rinva * (reinterpret_cast<const float*>(QSEL(wpack) + a.bias_off[l]) + HP)[1];
        }
        const __amdgpu_buffer_rsrc_t ao = slab_rsrc(a.saved + a.agg_off[l]);
        const unsigned ao_off = (rvalid && a.need_backward) ? rowoff : kOob;
        auto fillA = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
            if constexpr (Q < kDma) dmaA(qq);
            else if constexpr (Q < kDma + NT && !JOBS) buf_store(ag[Q - kDma], ao, ao_off + 64 * (Q - kDma));
        };
        contract_half_fill<NT, MATH>(wbuf, lane, ag, acc, rsa, fillA);
        static_for<kTail, kFill>(fillA);
        QSTAMP(0, l, 5);
        {   // epilogue: (bias,) ReLU, new rows -> registers and LDS
            f32x4* xr = reinterpret_cast<f32x4*>(xbuf + lrow * XS) + g;
            const f32x4* bl = reinterpret_cast<const f32x4*>(s_bias) + g;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                f32x4 v = acc[t];
                if constexpr (MATH == 1) { v *= rinv; v += bl[4 * t]; }
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) v[q4] = relu_raw(v[q4]);
                if constexpr (MATH == 1) v *= validf;              // pad rows stay exactly zero
                xs[t] = v;
                xr[4 * t] = v;
            }
        }
        wait_vmem();
        QSTAMP(0, l, 6);
        lds_barrier();     // barrier 2: new rows + half B = W_r(l+1) visible; half A free
        QSTAMP(0, l, 7);
    }
    if constexpr (!JOBS) {   // the last layer's rows (the only layer when L == 1)
        if (a.L > 1) publish_xmax(a.L - 1);
        const __amdgpu_buffer_rsrc_t ylast = slab_rsrc(a.acts + slab * (a.L - 1));
        const unsigned ylast_off = acts_off(a.L - 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) buf_store(xs[t], ylast, ylast_off + 64 * t);
    }

    // ---- head tail (scratch aliases the weight halves, free after the last barrier) ----
    float* sc = reinterpret_cast<float*>(lds + LD::off_scr_tail);
    float* s_w = sc;                 // [128] advantage weights
    float* s_pool = sc + 128;        // [4*128]
    float* s_z = sc + 640;           // [64]
    float* s_red = sc + 704;         // [8]
    float* s_misc = sc + 712;        // [0] = tanh(v)
    float* s_mx = sc + 768;          // [3][128]
    float* s_mn = sc + 1152;         // [3][128]
    float* s_sm = sc + 1536;         // [3][128]
    int* s_ax = reinterpret_cast<int*>(sc + 1920);   // [3][128]
    int* s_an = reinterpret_cast<int*>(sc + 2304);   // [3][128]
    const int H2 = H / 2, H4 = 4 * H;
    if (tid < 128) s_w[tid] = tid < H ? QSEL(lin_w)[tid] : 0.f;
    // the tail's small global operands are requested here, one round trip for all of them, instead of one each at the point
    // of use (four exposed round trips on a path with no other work to hide them)
    const float lin_b0 = QSEL(lin_b)[0];
    const int vk_ = tid >> 3;
    const float v0b_k = (QMODE != 2 && vk_ < H2) ? QSEL(v0_b)[vk_] : 0.f;
    const float v1w_l = (QMODE != 2 && wave == 0 && lane < H2) ? QSEL(v1_w)[lane] : 0.f;
    const float v1b_0 = QMODE != 2 ? QSEL(v1_b)[0] : 0.f;
    const bool td_on = !JOBS && a.td_sel != nullptr && QMODE == 0;
    const long long td_s = td_on ? a.td_sel[gi] : -1;
    const float td_t = td_on ? a.td_tgt[gi] : 0.f;
    const float td_wg = (td_on && a.td_w) ? a.td_w[gi] : 1.f;
    if constexpr (kCarry) { cy.e0t = cy.rowptr_t[r0]; cy.e1t = cy.rowptr_t[r1]; }
    __syncthreads();
    // advantages from the registers: partial dot over this lane's chunks, reduce over the 4 lanes of the row
    float adv = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const f32x4 w = reinterpret_cast<const f32x4*>(s_w)[4 * t + g];
        adv += xs[t][0] * w[0] + xs[t][1] * w[1] + xs[t][2] * w[2] + xs[t][3] * w[3];
    }
    adv += __shfl_xor(adv, 16);
    adv += __shfl_xor(adv, 32);
    adv += lin_b0;
    const float tadv = 2.f * tanhf(adv);
    if (g == 0 && rvalid) {
        if constexpr (!JOBS) a.adv_raw[grow] = adv;
        if (QMODE == 2) QSEL(q)[grow] = tadv;
    }
    if (QMODE == 2) return;
    {   // sum of 2tanh(adv) over the graph: lanes g==0 of valid rows; fixed-shape tree
        float v = (g == 0 && rvalid) ? tadv : 0.f;
        v = wave_sum(v);
        if (lane == 0) s_red[wave] = v;
    }
    // value-MLP weights -> registers now (the loads fly during pooling): thread (k = tid / 8, part = tid % 8) takes hidden
    // unit k (up to 64) and the 16-byte column groups part, part + 8, ... of its 4H-wide row (H groups, H <= 112: 14 loads)
    constexpr int kVQ = 14;
    const int vk = tid >> 3, vpart = tid & 7;
    f32x4 wv[kVQ];
    {
        const f32x4* wrow = reinterpret_cast<const f32x4*>(QSEL(v0_w) + (size_t)vk * H4);
#pragma unroll
        for (int j = 0; j < kVQ; ++j) {
            const int q = vpart + 8 * j;
            wv[j] = (vk < H2 && q < H) ? wrow[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    // pooling straight from the LDS rows: column c = tid&127, four row phases
    {
        const int c = tid & 127, ph = tid >> 7;
        float sum = 0.f, mx = -INFINITY, mn = INFINITY;
        int ax = -1, an = -1;
        if (c < H) {
            for (int row = ph; row < cnt; row += 4) {
                const float v = xbuf[row * XS + c];
                sum += v;
                if (v > mx) { mx = v; ax = row; }
                if (v < mn) { mn = v; an = row; }
            }
        }
        if (ph > 0) {
            const int o = (ph - 1) * 128 + c;
            s_sm[o] = sum; s_mx[o] = mx; s_mn[o] = mn; s_ax[o] = ax; s_an[o] = an;
        }
        __syncthreads();
        if (ph == 0 && c < H) {
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const int o = p * 128 + c;
                sum += s_sm[o];
                const float mx1 = s_mx[o], mn1 = s_mn[o];
                const int ax1 = s_ax[o], an1 = s_an[o];
                if (ax1 >= 0 && (ax < 0 || mx1 > mx || (mx1 == mx && ax1 < ax))) { mx = mx1; ax = ax1; }
                if (an1 >= 0 && (an < 0 || mn1 < mn || (mn1 == mn && an1 < an))) { mn = mn1; an = an1; }
            }
            if (cnt == 0) { mx = 0.f; mn = 0.f; }
            const float mean = sum / (float)max(cnt, 1);
            s_pool[c] = sum; s_pool[H + c] = mx; s_pool[2 * H + c] = mn; s_pool[3 * H + c] = mean;
            if constexpr (!JOBS) {
                float* pg = a.pooled + (size_t)gi * H4;
                pg[c] = sum; pg[H + c] = mx; pg[2 * H + c] = mn; pg[3 * H + c] = mean;
                a.amax[(size_t)gi * H + c] = ax >= 0 ? r0 + ax : -1;
                a.amin[(size_t)gi * H + c] = an >= 0 ? r0 + an : -1;
            }
        }
    }
    __syncthreads();
    {
        f32x4 p4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kVQ; ++j) {
            const int q = vpart + 8 * j;
            if (q < H) p4 += wv[j] * reinterpret_cast<const f32x4*>(s_pool)[q];
        }
        float p = (p4[0] + p4[1]) + (p4[2] + p4[3]);
        p = oct_sum(p);          // over the 8 lanes that share the hidden unit
        if (vpart == 0 && vk < H2) {
            const float zz = fmaxf(p + v0b_k, 0.f);
            s_z[vk] = zz;
            if constexpr (!JOBS) a.z[(size_t)gi * H2 + vk] = zz;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float p = lane < H2 ? v1w_l * s_z[lane] : 0.f;
        p = wave_sum(p);
        if (lane == 0) {
            const float v = p + v1b_0;
            if constexpr (!JOBS) a.vraw[gi] = v;
            s_misc[0] = tanhf(v);
        }
    }
    __syncthreads();
    float adv_total = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) adv_total += s_red[w];
    const float mean_adv = adv_total / (float)max(cnt, 1);
    const float V = s_misc[0];
    if constexpr (!JOBS) { if (QMODE == 1 && tid == 0) a.out_v[gi] = V; }
    const float qv = (QMODE == 0 ? V : 0.f) + tadv - mean_adv;
    if (g == 0 && rvalid) QSEL(q)[grow] = qv;
    if (td_on) {
        // loss = mean_g w_g l(Q[sel_g] - target_g) with td_loss.h's per-entry expressions; the mean over the graphs is summed
        // from td_loss_part by the backward's reduce launch
        if (g == 0 && rvalid) {
            float d = 0.f;
            if ((long long)grow == td_s) {
                const float e = qv - td_t;
                a.td_out[gi] = e;
                a.td_loss_part[gi] = td_wg * td_term(e, a.td_loss_fn);
                const float dl = td_dterm(e, a.td_loss_fn);
                d = (1.f / (float)a.b) * td_wg * dl;
            }
            a.td_dq[grow] = d;
        }
        if (tid == 0 && (td_s < (long long)r0 || td_s >= (long long)r1)) {
            // the selected node is not a row of this graph (contract of the fused form): flag AND poison
            atomicOr(a.status, 16);
            a.td_out[gi] = __builtin_nanf("");
            a.td_loss_part[gi] = __builtin_nanf("");
        }
    }
    if constexpr (kCarry) {
        cy.r0 = r0; cy.r1 = r1; cy.idg = idg;
#pragma unroll
        for (int t = 0; t < NT; ++t) cy.xs[t] = xs[t];
    }
    QSTAMP(0, 0, 2);
