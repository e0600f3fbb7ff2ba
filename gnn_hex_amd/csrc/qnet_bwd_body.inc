// Body of the per-graph backward data chain, included into qnet_bwd_kernel and qnet_step_kernel (qnet_fused_kernels.h).  In
// scope: the arguments `a`, NT and MATH.  Kept as text for the reason given in qnet_fwd_body.inc.
    using LD = QLds<NT>;
    constexpr int HP = LD::HP, XS = LD::XS, kHalf = LD::kHalf;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    f32x4* wbuf = reinterpret_cast<f32x4*>(lds + LD::off_w);
    float* dbuf = reinterpret_cast<float*>(lds + LD::off_x);
    const unsigned short* s_rp = reinterpret_cast<const unsigned short*>(lds + LD::off_rp);
    const unsigned char* s_col = reinterpret_cast<const unsigned char*>(lds + LD::off_col);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int gi = blockIdx.x;
    QSTAMP(1, 0, 0);
    const int H = a.H, L = a.L;
    // Requested before anything that depends on the graph (round 4): the top layer's W_r part (staged into half B below) and this
    // thread's share of the value MLP's first-layer weights (d pooled = v0_w^T dz, three barriers further down) -- their round
    // trips then overlap the chain gptr -> rowptr -> columns instead of following it.
    constexpr int kStage = (kHalf + 511) / 512;
    f32x4 wstg[kStage];
    if (L > 1) {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.wpack + a.bwd_off[L - 1]) + kHalf;
#pragma unroll
        for (int k = 0; k < kStage; ++k) {
            const int i = tid + 512 * k;
            if (i < kHalf) wstg[k] = src[i];
        }
    }
    constexpr int kVW = 14;           // H / 2 <= 56 hidden units over four k phases
    f32x4 vw[kVW];
    {
        const int cq = tid & 127, kg = tid >> 7;
        const f32x4* wq = reinterpret_cast<const f32x4*>(a.v0_w) + cq;
#pragma unroll
        for (int j = 0; j < kVW; ++j) {
            const int k = kg + 4 * j;
            vw[j] = (a.mode != 2 && cq < H && k < H / 2) ? wq[(size_t)k * H] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const int r0 = kCarry ? cy.r0 : a.gptr[gi], r1 = kCarry ? cy.r1 : a.gptr[gi + 1];
    const int cnt = r1 - r0;
    if (cnt > kRows) { if (tid == 0) atomicOr(a.status, 2); return; }
    const int lrow = wave * 16 + r;
    const bool rvalid = lrow < cnt;
    const bool wactive = wave * 16 < cnt;
    const bool spare = cnt <= kRows / 2;            // workgroup-uniform: waves 4-7 own no rows (dma_share)
    const int grow = r0 + lrow;
    const int H2 = H / 2;
    const size_t slab = (size_t)a.n * HP;
    // Every global value the head-tail backward needs is requested here, before the CSR / weight staging, so that the
    // chain below waits for ONE memory round trip instead of one per barrier-separated step.
    const float dq_t = tid < cnt ? a.dq[r0 + tid] : 0.f;
    const float advr_t = tid < cnt ? a.adv_raw[r0 + tid] : 0.f;
    const float linw_t = (tid < 128 && tid < H) ? a.lin_w[tid] : 0.f;
    float vraw_g = 0.f, doutv_g = 0.f, z_t = 0.f, v1w_t = 0.f;
    int ax_t = -1, an_t = -1;
    if (a.mode != 2) {
        vraw_g = a.vraw[gi];
        if (a.mode != 0) doutv_g = a.d_out_v[gi];
        if (tid < H2) { z_t = a.z[(size_t)gi * H2 + tid]; v1w_t = a.v1_w[tid]; }
        if (tid < H) { ax_t = a.amax[(size_t)gi * H + tid]; an_t = a.amin[(size_t)gi * H + tid]; }
    }
    const float idg = kCarry ? cy.idg : (rvalid ? a.invdeg[grow] : 0.f);     // (used from the first layer on: requested with everything else)
    f32x4 ytop[NT];      // y rows of the top layer: operand of the advantage-linear gradient and of the first ReLU mask
    if constexpr (kCarry) {
#pragma unroll
        for (int t = 0; t < NT; ++t) ytop[t] = cy.xs[t];
    } else {
        const f32x4* yr = reinterpret_cast<const f32x4*>(a.acts + slab * (L - 1) + (size_t)grow * HP) + g;
#pragma unroll
        for (int t = 0; t < NT; ++t) ytop[t] = rvalid ? yr[4 * t] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int e0 = kCarry ? cy.e0t : a.rowptr_t[r0], ne = (kCarry ? cy.e1t : a.rowptr_t[r1]) - e0;
    const bool csr_lds = load_csr<NT>(lds, a.rowptr_t, a.col_t, r0, cnt, e0, ne, a.status);
    float* s_max = reinterpret_cast<float*>(lds + LD::off_max);      // per-wave maxima (math 1)
    if (tid < 16) s_max[tid] = 0.f;
    if (tid < XS) dbuf[kRows * XS + tid] = 0.f;                      // the gather's filler row

    // stage the W_r part of the top layer into half B (the self half runs first; everything else arrives by LDS-DMA)
    if (L > 1) {
#pragma unroll
        for (int k = 0; k < kStage; ++k) { const int i = tid + 512 * k; if (i < kHalf) wbuf[kHalf + i] = wstg[k]; }
    }

    // ---- head tail backward; scratch aliases dbuf (not written before the first barrier A) ----
    float* sc = dbuf;
    float* s_w = sc;                  // [128]
    float* s_dp = sc + 128;           // [4*128]
    float* s_dz = sc + 640;           // [64]
    float* s_red = sc + 704;          // [8]
    float* s_dar = sc + 768;          // [128]
    int* s_ax = reinterpret_cast<int*>(sc + 896);    // [128] local row of the max
    int* s_an = reinterpret_cast<int*>(sc + 1024);
    float* s_lin = sc + 1152;         // [8][HP+1]
    float* s_part = sc + ((1152 + 8 * (HP + 1) + 3) & ~3);   // [3][HP] float4 partial sums of the value-MLP product (narrow widths: the row buffer is small)
    if (tid < 128) s_w[tid] = linw_t;
    float mean_dq = 0.f;
    const float inv_cnt = 1.f / (float)max(cnt, 1);
    if (a.mode != 2) {
        float ps = wave_sum(dq_t);
        if (lane == 0) s_red[wave] = ps;
        if (tid < H) {
            s_ax[tid] = ax_t >= 0 ? ax_t - r0 : -1;
            s_an[tid] = an_t >= 0 ? an_t - r0 : -1;
        }
        __syncthreads();
        float sdq = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) sdq += s_red[w];
        mean_dq = sdq * inv_cnt;
        const float dV = a.mode == 0 ? sdq : doutv_g;
        const float dv = dV * sech2f(vraw_g);
        if (tid == 0) a.dvr[gi] = dv;
        if (tid < H2) {
            const float d = z_t > 0.f ? v1w_t * dv : 0.f;
            s_dz[tid] = d;
            a.dz[(size_t)gi * H2 + tid] = d;
        }
        __syncthreads();
        // d pooled = v0_w^T dz  ([H2] x [H2][4H]): 16-byte column groups x four k phases, every load independent
        {
            const int cq = tid & 127, kg = tid >> 7;
            f32x4 p4 = f32x4{0.f, 0.f, 0.f, 0.f};
            if (cq < H) {
#pragma unroll
                for (int j = 0; j < kVW; ++j) { const int k = kg + 4 * j; if (k < H2) p4 += vw[j] * s_dz[k]; }
            }
            if (kg > 0 && cq < H) reinterpret_cast<f32x4*>(s_part)[(kg - 1) * HP + cq] = p4;
            __syncthreads();
            if (kg == 0 && cq < H) {
                const f32x4* sp = reinterpret_cast<const f32x4*>(s_part) + cq;
                p4 += sp[0]; p4 += sp[HP]; p4 += sp[2 * HP];      // fixed order: deterministic
                // s_dp = [sum | max | min | mean][128]: each pooled block on its own 16-byte aligned row
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int f = 4 * cq + j; s_dp[(f / H) * 128 + f % H] = p4[j]; }
            }
        }
    }
    if (tid < kRows) {
        float dar = 0.f;
        if (tid < cnt) {
            dar = (dq_t - mean_dq) * 2.f * sech2f(advr_t);
            a.dadv[r0 + tid] = dar;
        }
        s_dar[tid] = dar;
    }
    __syncthreads();
    const NbrRegs nbr = csr_lds ? load_nbrs<XS>(s_rp, s_col, lrow, rvalid, g)
                                : load_nbrs_global<XS>(a.rowptr_t, a.col_t, r0, cnt, e0, lrow, rvalid, g);

    // gradient w.r.t. the top layer's output, in the chained lane layout; advantage-linear partial alongside
    f32x4 gx[NT];
    {
        const float dar = s_dar[lrow];
        float lacc[NT * 4];
        typedef int i32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const f32x4 w = reinterpret_cast<const f32x4*>(s_w)[4 * t + g];
            const f32x4 yv = ytop[t];
            // this lane's four columns of the pooled gradients in 16-byte reads (as scalars: 168 ds_read_b32 per lane)
            const f32x4 d_sum = reinterpret_cast<const f32x4*>(s_dp)[4 * t + g];
            const f32x4 d_max = reinterpret_cast<const f32x4*>(s_dp + 128)[4 * t + g];
            const f32x4 d_min = reinterpret_cast<const f32x4*>(s_dp + 256)[4 * t + g];
            const f32x4 d_mean = reinterpret_cast<const f32x4*>(s_dp + 384)[4 * t + g];
            const i32x4 axv = reinterpret_cast<const i32x4*>(s_ax)[4 * t + g];
            const i32x4 anv = reinterpret_cast<const i32x4*>(s_an)[4 * t + g];
            f32x4 v;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int c = 16 * t + 4 * g + q4;
                float s = dar * w[q4];
                if (a.mode != 2 && c < H) {
                    s += d_sum[q4] + d_mean[q4] * inv_cnt;
                    if (axv[q4] == lrow) s += d_max[q4];
                    if (anv[q4] == lrow) s += d_min[q4];
                }
                v[q4] = (rvalid && c < H) ? s : 0.f;
                lacc[4 * t + q4] = dar * yv[q4];
            }
            gx[t] = v;
        }
        // d lin_w[c] partial = sum_rows dar*h[row][c]: reduce over the 16 rows of the wave, then over waves
        // (DPP row operations: the 16 rows of a wave are the 16 lanes of one DPP row; as __shfl_xor this butterfly was 116
        // ds_bpermute per wave and took 7.7 us of the prologue)
        float bacc = row16_sum(g == 0 ? dar : 0.f);
#pragma unroll
        for (int k = 0; k < NT * 4; ++k) lacc[k] = row16_sum(lacc[k]);
        if (r == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) s_lin[wave * (HP + 1) + 16 * t + 4 * g + q4] = lacc[4 * t + q4];
            if (g == 0) s_lin[wave * (HP + 1) + HP] = bacc;
        }
    }
    __syncthreads();
    if (tid <= HP) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) s += s_lin[w * (HP + 1) + tid];
        a.lin_part[(size_t)gi * (HP + 1) + tid] = s;
    }
    __syncthreads();   // scratch consumed; dbuf may be overwritten from here on

    // ---- layer chain, in the forward kernel's shape ----
    //   dL/dy_{l-1} = [ T(G_l / deg) | G_l ] [W_l ; W_r]   (T = gather over the transposed CSR; linear, so the gather is
    //   moved in front of the contraction): per layer  gather from LDS -> K-half over the W_l part -> barrier ->
    //   K-half over the W_r part with G_l from registers -> mask by y_{l-1} -> publish G_{l-1} (global + LDS) -> barrier.
    // gx = dL/dy_l, yv = this lane's y_l chunks  ->  G_l = gx * [y_l > 0]; (l >= 1) G_l / deg goes to this lane's LDS row
    // for the neighbours' gathers.  The y rows are loaded by the caller a whole layer ahead into iteration-local
    // registers (a loop-carried prefetch made hipcc wait for the load in place).  store_G() then writes G_l for the
    // weight-gradient GEMM; it is a separate step so that the weight-half LDS writes can sit between the two (see the
    // forward kernel: a wait for staged loads placed after global stores also waits for the stores).
    const unsigned rowoff = (unsigned)grow * (HP * 4) + 16 * g;      // byte offset of this lane's slot inside a [n][HP] slab
    const unsigned lane16 = 16 * lane;
    const unsigned rowoff_v = rvalid ? rowoff : kOob;    // pad rows: stores dropped, loads return zeros
    // (no `if (rvalid)` region: a pad row's y loads return zeros, so the mask alone zeroes its gradient, and the tap store
    // drops out of range -- a divergent region around the mask cost a select or a copy per register at its merge)
    auto mask_rows = [&](const int l, const f32x4 (&yv)[NT]) {
        if (a.d_embeds && l == a.body_layers - 1) {
            const __amdgpu_buffer_rsrc_t de = slab_rsrc(a.d_embeds);
#pragma unroll
            for (int t = 0; t < NT; ++t) buf_store(gx[t], de, rowoff_v + 64 * t);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) gx[t][q4] = yv[t][q4] > 0.f ? gx[t][q4] : 0.f;
        }
        if (l > 0) {
            f32x4* dr = reinterpret_cast<f32x4*>(dbuf + lrow * XS) + g;
#pragma unroll
            for (int t = 0; t < NT; ++t) dr[4 * t] = gx[t] * idg;
            if constexpr (MATH == 1) {
                if (a.gmax) {
                    const float wm = rows_max16(row_max4(frag_absmax<NT>(gx, 0.f)));
                    if (lane == 0) s_max[wave] = wm;
                }
            }
        }
    };
    auto store_G = [&](const int l, const int t) {       // chunk t of this lane's row of G_l (held in gx)
        buf_store(gx[t], slab_rsrc(a.G + slab * l), rowoff_v + 64 * t);
    };
    QSTAMP(1, 0, 1);
    if (wactive) {
        mask_rows(L - 1, ytop);
#pragma unroll
        for (int t = 0; t < NT; ++t) store_G(L - 1, t);
    }
    lds_barrier();
    QSTAMP(1, 0, 2);
    // Per layer two phases in the forward kernel's shape (fillers between the MFMA groups):
    //   phase S: G_l (registers) x W_r part (half B); fillers = transposed LDS gather of G_l / deg, the deferred store of
    //            G_l, LDS-DMA of the W_l part into half A                                          -> barrier 1
    //   phase A: gathered rows x W_l part (half A); fillers = loads of y_{l-1}, LDS-DMA of layer l-1's W_r part into
    //            half B; then mask by y_{l-1}, G_{l-1} / deg -> LDS                                -> barrier 2
    constexpr int kGaps = Gaps<NT, MATH>::value;
    constexpr int kDma = (NT * NT + 7) / 8;
    constexpr int kFill = kDma + NT;
    constexpr int kTail = kFill > kGaps ? kGaps : kFill;
    const unsigned lds_w = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(lds + LD::off_w);
    for (int l = L - 1; l >= 1; --l) {
        QSTAMP(1, l, 0);
        const f32x4* wsrc = reinterpret_cast<const f32x4*>(a.wpack + a.bwd_off[l]);
        const bool more = l - 1 >= 1;
        const f32x4* nsrc = reinterpret_cast<const f32x4*>(a.wpack + a.bwd_off[more ? l - 1 : l]) + kHalf;
        if constexpr (MATH == 1) {
            if (a.gmax && tid == 0) {   // layer maximum of |G_l| over this graph -> global (order-independent)
                float mm = 0.f;
#pragma unroll
                for (int w8 = 0; w8 < 8; ++w8) mm = fmaxf(mm, s_max[w8]);
                atomicMax(a.gmax + l, __builtin_bit_cast(unsigned, mm));
            }
        }
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
        if (!wactive) {      // a wave without rows only moves its weight pieces (own straight path, as in the forward kernel)
            static_for<0, kDma>(dmaS);
            wait_vmem();
            lds_barrier();
            static_for<0, kDma>(dmaA);
            wait_vmem();
            lds_barrier();
            continue;
        }
        f32x4 acc[NT], ag[NT];
        if constexpr (MATH == 1) {
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float rs = 1.f, rinv = 1.f, mx = 0.f;
        f32x4 tb[GatherLand<NT, MATH>::value][NT];
        if constexpr (MATH == 1) { mx = row_max4(frag_absmax<NT>(gx, 0.f)); row_scale(mx, rs, rinv); }
        // ---- phase S ----
        const __amdgpu_buffer_rsrc_t gcur = slab_rsrc(a.G + slab * l);
        const unsigned gcur_off = l < L - 1 ? rowoff_v : kOob;      // the top layer's G was stored ahead of the loop
        auto fillS = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
            gather_gap<NT, Q, kGaps, MATH>(dbuf, nbr, ag, tb);
            if constexpr (Q < kDma) dmaS(qq);
            else if constexpr (Q < kDma + NT) buf_store(gx[Q - kDma], gcur, gcur_off + 64 * (Q - kDma));
        };
        contract_half_fill<NT, MATH, MATH == 0>(wbuf + kHalf, lane, gx, acc, rs, fillS);
        static_for<kTail, kFill>(fillS);
        if (nbr.wlong) {      // (wave-uniform; pad rows: eb == ee)
            if (csr_lds) gather_lds<NT, XS>(dbuf, s_col, nbr.eb, nbr.ee, g, ag);
            else gather_global_tail<NT, XS>(dbuf, a.col_t, r0, cnt, e0 + nbr.eb, e0 + nbr.ee, g, ag);
        }
        QSTAMP(1, l, 1);
        wait_vmem();
        QSTAMP(1, l, 3);
        lds_barrier();     // barrier 1: half A = W_l part; every gather of this layer is done (dbuf free); half B free
        QSTAMP(1, l, 4);
        // ---- phase A ----
        float rsa = 1.f;
        if constexpr (MATH == 1) {   // own power-of-two row scale for the gathered rows, exact carry of the self half's sums
            float ma = row_max4(frag_absmax<NT>(ag, 0.f));
            ma = fmaxf(ma, mx * 0x1p-40f);
            float rinva;
            row_scale(ma, rsa, rinva);
            const float carry = rsa * rinv;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] *= carry;
            rinv = rinva * (reinterpret_cast<const float*>(a.wpack + a.bias_off[l]) + HP)[1];
        }
        const __amdgpu_buffer_rsrc_t yr = slab_rsrc(a.acts + slab * (l - 1));
        f32x4 yl[NT];        // y_{l-1} rows for this iteration's closing mask
        auto fillA = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
            if constexpr (Q < NT) {
                load_guard<MATH>();
                yl[Q] = buf_load(yr, rowoff_v + 64 * Q);
            } else if constexpr (Q < NT + kDma) {
                dmaA(std::integral_constant<int, Q - NT>{});
            }
        };
        contract_half_fill<NT, MATH>(wbuf, lane, ag, acc, rsa, fillA);
        static_for<kTail, kFill>(fillA);
        QSTAMP(1, l, 5);
#pragma unroll
        for (int t = 0; t < NT; ++t) gx[t] = MATH == 1 ? acc[t] * rinv : acc[t];
        mask_rows(l - 1, yl);
        wait_vmem();
        QSTAMP(1, l, 6);
        lds_barrier();     // barrier 2: G_{l-1} rows + half B visible; half A free
        QSTAMP(1, l, 7);
    }
    if (wactive && L > 1) {
#pragma unroll
        for (int t = 0; t < NT; ++t) store_G(0, t);
    }
    // ---- raw first layer: this graph's share of dW_0 = G_0^T [agg0 | x0 | 1], reduced over the graphs afterwards ----
    if (a.first_part) {
        __syncthreads();             // every wave's last gather is done: dbuf and the weight halves are free
        // F = [agg0(8) | x0(8) | 1 | 0...] per row, 48-float rows (stride == 16 mod 32: conflict-free fragment reads)
        float* s_f = reinterpret_cast<float*>(lds + LD::off_scr_bwd0);
        {
            f32x4* dr = reinterpret_cast<f32x4*>(dbuf + lrow * XS) + g;
#pragma unroll
            for (int t = 0; t < NT; ++t) dr[4 * t] = rvalid ? gx[t] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (tid < kRows) {
            f32x4* fr = reinterpret_cast<f32x4*>(s_f + tid * 48);
            f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0, x0 = a0, x1 = a0, one = a0;
            if (tid < cnt) {
                const f32x4* ar = reinterpret_cast<const f32x4*>(a.agg0 + (size_t)(r0 + tid) * kSmallCin);
                a0 = ar[0]; a1 = ar[1];
                const float* xr = a.x + (size_t)(r0 + tid) * a.x_stride;
#pragma unroll
                for (int q = 0; q < 4; ++q) { x0[q] = q < a.c_in ? xr[q] : 0.f; x1[q] = 4 + q < a.c_in ? xr[4 + q] : 0.f; }
                one[0] = 1.f;
            }
            fr[0] = a0; fr[1] = a1; fr[2] = x0; fr[3] = x1; fr[4] = one;
            fr[5] = f32x4{0.f, 0.f, 0.f, 0.f}; fr[6] = fr[5]; fr[7] = fr[5];
        }
        __syncthreads();
        if (wave < NT) {
            // dW_0^T tile [c (2 x 16)][o = 16 wave ..] = F^T G_0 over the 128 rows: exact fp32 MFMA, two interleaved chains
            f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll 8
            for (int k = 0; k < kRows / 4; ++k) {
                const int row = 4 * k + g;
                const float bv = dbuf[row * XS + 16 * wave + r];
                acc0 = mfma16x16x4(s_f[row * 48 + r], bv, acc0);
                acc1 = mfma16x16x4(s_f[row * 48 + 16 + r], bv, acc1);
            }
            float* out = a.first_part + (size_t)gi * 17 * HP + 16 * wave + r;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[(size_t)(4 * g + j) * HP] = acc0[j];
            if (g == 0) out[(size_t)16 * HP] = acc1[0];
        }
    }
    QSTAMP(1, 0, 3);
