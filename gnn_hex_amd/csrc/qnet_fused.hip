// C ABI of the fused per-graph path + the exact-fp32 instantiations (kernels: qnet_fused_kernels.h).
#include "qnet_fused_kernels.h"
#include "hexgnn_reduce.h"

namespace hexgnn {

int launch_qfwd_math(int nt, int math, const QFwdArgs& a, hipStream_t st) {
    if (math == 1) return launch_qfwd_split(nt, a, st);
    HEXGNN_NT_SWITCH7(nt, (launch_qfwd_m<NT_, 0>(a, st)));
    return HEXGNN_OK;
}
int launch_qbwd_math(int nt, int math, const QBwdArgs& a, hipStream_t st) {
    if (math == 1) return launch_qbwd_split(nt, a, st);
    HEXGNN_NT_SWITCH7(nt, (launch_qbwd_m<NT_, 0>(a, st)));
    return HEXGNN_OK;
}


// ---- ONE launch for every reduction that turns the backward's partial results into parameter gradients --------------
// roles by block range (256 threads each):
//   R0  hidden-layer dW / db: sum of the S row-slice slabs written by sage_dw(16)_kernel            (fixed order over s)
//   R1  raw first layer dW / db: sum over graphs of the per-graph partials of qnet_bwd_kernel        (wave per output)
//   R2  advantage Linear: sum over graphs of lin_part                                               (wave per output)
//   R3  value MLP: d_v0_w = dz^T pooled, d_v0_b, d_v1_w, d_v1_b                                     (as head_value_wgrad_kernel)
// Every sum has a fixed shape => bit-reproducible.  Replaces five launches of the layered path.
struct GradReduceArgs {
    float* dwl[kMaxLayers]; float* dbl[kMaxLayers]; float* dwr[kMaxLayers];   // hidden layers (index = hidden layer)
    const float* part; int S, hp, H, nh, blk_per_layer, per;
    const float* first_part; int b, c_in; float* dwl0; float* dbl0; float* dwr0;
    const float* lin_part; float* d_lin_w; float* d_lin_b;
    const float* dz; const float* dvr; const float* pooled; const float* z;
    float* d_v0_w; float* d_v0_b; float* d_v1_w; float* d_v1_b;
    int n0, n1, n2, n3, nbx3;
    // R4 (one block, a backward with td_loss): loss = (sum over the b graphs of loss_part) / b, by tree_mean_256
    const float* loss_part; float* loss;
};

__global__ __launch_bounds__(256) void qnet_grad_reduce_kernel(GradReduceArgs a) {
    int blk = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, hp = a.hp;
    if (blk == a.n0 + a.n1 + a.n2 + a.n3) {      // ---- R4: the TD loss's mean over the graphs
        __shared__ float lred[256];
        float acc = 0.f;
        for (int j = tid; j < a.b; j += 256) acc += a.loss_part[j];
        const float mean = tree_mean_256(acc, lred, a.b);
        if (tid == 0) a.loss[0] = mean;
        return;
    }
    if (blk < a.n0) {                     // ---- R0: slice slabs -> dW_l / dW_r / db of one hidden layer
        // one thread per float4 of the [hp][2hp] slab (+ the bias row), S independent 16-byte loads in flight
        // (blk_per_layer x hidden layers ~ two workgroups per CU, every one with the same share `per` of the slab: 400 blocks
        // of 256 float4 left 144 CUs with twice the bytes of the other 112, and the kernel is bound by bytes per CU)
        const int li = blk / a.blk_per_layer, idx = (blk % a.blk_per_layer) * a.per + tid;
        const int q_row = 2 * hp / 4, q_w = hp * q_row, q_all = q_w + hp / 4;
        if (tid >= a.per || idx >= q_all) return;
        const size_t slab_sz = (size_t)hp * (2 * hp + 1);
        const f32x4* p = reinterpret_cast<const f32x4*>(a.part + (size_t)li * a.S * slab_sz) + idx;   // slab_sz % 4 == 0
        f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int s = 0; s < a.S; ++s) sum += p[(size_t)s * (slab_sz / 4)];
        if (idx < q_w) {
            const int o = idx / q_row, c0 = (idx % q_row) * 4;
            if (o >= H) return;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j;
                if (c < H) a.dwl[li][o * H + c] = sum[j];
                else if (c >= hp && c - hp < H) a.dwr[li][o * H + (c - hp)] = sum[j];
            }
        } else {
            const int o0 = (idx - q_w) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (o0 + j < H) a.dbl[li][o0 + j] = sum[j];
        }
        return;
    }
    blk -= a.n0;
    if (blk < a.n1) {                     // ---- R1
        const int per = 2 * a.c_in + 1;
        const int idx = blk * 4 + wave;
        if (idx >= H * per) return;
        const int o = idx / per, c = idx % per;
        const int q = c < a.c_in ? c : (c < 2 * a.c_in ? kSmallCin + (c - a.c_in) : 2 * kSmallCin);
        float sum = 0.f;
        for (int g = lane; g < a.b; g += 64) sum += a.first_part[((size_t)g * 17 + q) * hp + o];
        sum = wave_sum(sum);
        if (lane == 0) {
            if (c < a.c_in) a.dwl0[o * a.c_in + c] = sum;
            else if (c < 2 * a.c_in) a.dwr0[o * a.c_in + (c - a.c_in)] = sum;
            else a.dbl0[o] = sum;
        }
        return;
    }
    blk -= a.n1;
    if (blk < a.n2) {                     // ---- R2
        const int c = blk * 4 + wave;     // c in [0, H]  (H == bias)
        if (c > H) return;
        lin_part_column_sum(a.b, hp, H, a.lin_part, c, lane, a.d_lin_w, a.d_lin_b);
        return;
    }
    blk -= a.n2;
    {                                     // ---- R3
        // 16 columns x 16 graph phases per block (round 4): with 64 columns x 4 phases a thread walked 64 graphs one dependent
        // batch of loads after the other, and these blocks -- not the slab sums -- set the length of the launch
        const int H2 = H / 2, H4 = 4 * H;
        const int bx = blk % a.nbx3, k = blk / a.nbx3;
        const int cl = tid & 15, ph = tid >> 4;
        const int c = bx * 16 + cl;
        __shared__ float red16[16][17];
        float s = 0.f;
        if (c < H4) {
#pragma unroll 8
            for (int g = ph; g < a.b; g += 16) s += a.dz[(size_t)g * H2 + k] * a.pooled[(size_t)g * H4 + c];
        }
        red16[ph][cl] = s;
        __syncthreads();
        if (ph == 0 && c < H4) {
            float t = red16[0][cl];
#pragma unroll
            for (int j = 1; j < 16; ++j) t += red16[j][cl];          // fixed order: deterministic
            a.d_v0_w[(size_t)k * H4 + c] = t;
        }
        if (bx == 0) value_small_grads(a.b, H2, k, lane, wave, a.dz, a.dvr, a.z, a.d_v0_b, a.d_v1_w, a.d_v1_b);
    }
}

}  // namespace hexgnn

using namespace hexgnn;

namespace {
struct QPlan {
    StackPlan sp;
    HeadSaved hs;
    size_t head_saved_off, xmax_off, saved_total;
    BwdPlan bp;
    HeadWs hw;
    size_t ws_g_off, ws_part_off, ws_part0_off, ws_head_off, ws_first_off, ws_total;
};
int make_qplan(int n, int b, int c_in, int hidden, int L, QPlan* q) {
    int rc = make_plan(n, c_in, hidden, L, &q->sp);
    if (rc != HEXGNN_OK) return rc;
    if (!q->sp.small_first || q->sp.nt > 7 || hidden < 2) return HEXGNN_EUNSUPPORTED;
    q->hs = head_saved_plan(n, b, hidden);
    q->head_saved_off = align_up(q->sp.saved_bytes, 256);
    q->xmax_off = align_up(q->head_saved_off + q->hs.total, 256);     // per-layer maxima (math 1), kMaxLayers words
    q->saved_total = q->xmax_off + 2 * sizeof(unsigned) * kMaxLayers;   // xmax[kMaxLayers] then gmax[kMaxLayers]
    make_bwd_plan(n, q->sp, &q->bp);
    q->hw = head_ws_plan(n, b, hidden);
    const size_t slab = align_up(sizeof(float) * (size_t)n * q->sp.hp, 256);
    size_t off = 0;
    q->ws_g_off = off; off += slab * L;
    q->ws_part_off = off; off += align_up(sizeof(float) * dw_slab_count(L) * q->sp.hp * (2 * q->sp.hp + 1), 256);
    q->ws_part0_off = off; off += align_up(sizeof(float) * (size_t)q->bp.S0 * q->sp.hp * 17, 256);
    q->ws_head_off = off; off += q->hw.total;
    q->ws_first_off = align_up(off, 256); off = q->ws_first_off + sizeof(float) * (size_t)(b > 0 ? b : 1) * 17 * q->sp.hp;
    q->ws_total = off;
    return HEXGNN_OK;
}
}  // namespace

// math 1 + backward: the per-layer maxima (xmax | gmax) kept behind the saved tensors, zeroed by the pack's scale kernel
static unsigned* qfwd_maxima(const hexgnn_qnet_call& c, const QPlan& qp) {
    return (c.math == 1 && c.need_backward) ? (unsigned*)((char*)c.saved + qp.xmax_off) : nullptr;
}

// the forward kernel's arguments from the descriptor (one copy: every forward form and the chained step)
static void fill_qfwd_args(QFwdArgs& a, const hexgnn_qnet_call& c, const QPlan& qp) {
    a.n = c.n; a.b = c.b; a.c_in = c.c_in; a.H = c.hidden; a.L = c.total_layers; a.mode = c.mode; a.x_stride = c.x_stride;
    a.need_backward = c.need_backward;
    a.acts_layer = c.acts_layer;
    a.gptr = c.gptr; a.rowptr = c.rowptr; a.col = c.col; a.invdeg = c.invdeg; a.x = c.x;
    a.wpack = (const char*)c.wpack;
    for (int l = 0; l < c.total_layers; ++l) {
        a.fwd_off[l] = qp.sp.fwd_off[l]; a.bias_off[l] = qp.sp.bias_off[l]; a.agg_off[l] = qp.sp.agg_off[l];
    }
    a.acts = c.acts; a.saved = (char*)c.saved;
    a.lin_w = c.lin_w; a.lin_b = c.lin_b; a.v0_w = c.v0_w; a.v0_b = c.v0_b; a.v1_w = c.v1_w; a.v1_b = c.v1_b;
    char* hsv = (char*)c.saved + qp.head_saved_off;
    a.adv_raw = (float*)(hsv + qp.hs.adv_off); a.pooled = (float*)(hsv + qp.hs.pooled_off);
    a.amax = (int*)(hsv + qp.hs.amax_off); a.amin = (int*)(hsv + qp.hs.amin_off);
    a.z = (float*)(hsv + qp.hs.z_off); a.vraw = (float*)(hsv + qp.hs.v_off);
    a.q = c.q; a.out_v = c.out_v; a.status = c.status;
    a.xmax = qfwd_maxima(c, qp);
    a.td_sel = (const long long*)c.td_sel; a.td_tgt = c.td_target; a.td_w = c.td_weights; a.td_loss_fn = c.td_loss_fn;
    a.td_dq = c.td_dq; a.td_out = c.td_out; a.td_loss_part = c.td_loss_part;
}

// the backward data chain's arguments from the descriptor (one copy: every backward form and the chained step)
static void fill_qbwd_args(QBwdArgs& a, const hexgnn_qnet_call& c, const QPlan& qp) {
    char* ws = (char*)c.workspace;
    const char* sv = (const char*)c.saved;
    const char* hsv = sv + qp.head_saved_off;
    char* hws = ws + qp.ws_head_off;
    a.n = c.n; a.b = c.b; a.H = c.hidden; a.L = c.total_layers; a.mode = c.mode; a.body_layers = c.body_layers;
    a.gptr = c.gptr; a.rowptr_t = c.rowptr_t; a.col_t = c.col_t; a.invdeg = c.invdeg;
    a.wpack = (const char*)c.wpack;
    for (int l = 0; l < c.total_layers; ++l) { a.bwd_off[l] = qp.sp.bwd_off[l]; a.bias_off[l] = qp.sp.bias_off[l]; }
    a.acts = c.acts; a.lin_w = c.lin_w; a.v0_w = c.v0_w; a.v1_w = c.v1_w;
    a.adv_raw = (const float*)(hsv + qp.hs.adv_off); a.amax = (const int*)(hsv + qp.hs.amax_off);
    a.amin = (const int*)(hsv + qp.hs.amin_off); a.z = (const float*)(hsv + qp.hs.z_off);
    a.vraw = (const float*)(hsv + qp.hs.v_off);
    a.dq = c.dq; a.d_out_v = c.d_out_v; a.G = (float*)(ws + qp.ws_g_off); a.d_embeds = c.d_embeds;
    a.dadv = (float*)(hws + qp.hw.dadv_off); a.dz = (float*)(hws + qp.hw.dz_off);
    a.dvr = (float*)(hws + qp.hw.dvr_off); a.lin_part = (float*)(hws + qp.hw.part_off);
    a.status = c.status;
    a.x = c.x; a.x_stride = c.x_stride; a.c_in = c.c_in;
    a.agg0 = (const float*)(sv + qp.sp.agg_off[0]);
    a.first_part = (float*)(ws + qp.ws_first_off);
    // max |G_l| per layer (math 1): lives behind the forward's saved tensors, zeroed by the forward; a backward pass
    // repeated on the same saved state only re-maxes identical values
    a.gmax = c.math == 1 ? (unsigned*)(const_cast<char*>(sv) + qp.xmax_off) + kMaxLayers : nullptr;
}

// what the TD tail (td_sel set) wants besides td_sel: its buffers, a known loss, mode 0 with a backward to come
static bool td_tail_ok(const hexgnn_qnet_call& c) {
    return c.td_target && c.td_dq && c.td_out && c.td_loss_part && c.td_loss_fn >= 0 && c.td_loss_fn <= 1 && c.mode == 0 &&
           c.need_backward;
}

static int qnet_forward_impl(const hexgnn_qnet_call& c, hipStream_t st) {
    if (c.td_sel && !td_tail_ok(c)) return HEXGNN_EINVAL;
    if (c.n < 0 || c.b < 0 || c.mode < 0 || c.mode > 2 || c.math < 0 || c.math > 1) return HEXGNN_EINVAL;
    QPlan qp;
    int rc = make_qplan(c.n, c.b, c.c_in, c.hidden, c.total_layers, &qp);
    if (rc != HEXGNN_OK) return rc;
    // (wl = bl = wr = NULL: the weights were packed by hexgnn_csr_build_grouped_pack of this forward; exact fp32 only)
    const bool packed = !c.wl && !c.bl && !c.wr && c.math == 0;
    if (!c.gptr || (!packed && (!c.wl || !c.bl || !c.wr)) || !c.lin_w || !c.lin_b || !c.wpack || !c.saved || !c.status)
        return HEXGNN_EINVAL;
    if (c.mode != 2 && (!c.v0_w || !c.v0_b || !c.v1_w || !c.v1_b)) return HEXGNN_EINVAL;
    if (c.mode == 1 && !c.out_v) return HEXGNN_EINVAL;
    if (c.n > 0 && (!c.rowptr || !c.col || !c.invdeg || !c.x || !c.acts || !c.q)) return HEXGNN_EINVAL;
    if (c.x_stride < c.c_in) return HEXGNN_EINVAL;
    rc = launch_pack(qp.sp, c.c_in, c.hidden, c.wl, c.bl, c.wr, c.wpack, st, c.math, qfwd_maxima(c, qp));
    if (rc != HEXGNN_OK) return rc;
    if (c.b == 0) return check_launch();
    QFwdArgs a;
    fill_qfwd_args(a, c, qp);
    {
        KernelTimer kt(HEXGNN_K_QNET_FWD, st);
        rc = launch_qfwd_math(qp.sp.nt, c.math, a, st);
        if (rc != HEXGNN_OK) return rc;
    }
    return check_launch();
}

// forward, TD tail and the backward's data chain (on the tail's own td_dq) in one launch
static int qnet_step_impl(const hexgnn_qnet_call& c, hipStream_t st) {
    if (c.n <= 0 || c.b <= 0 || c.body_layers < 1 || c.body_layers > c.total_layers) return HEXGNN_EINVAL;
    if (!c.td_sel || !td_tail_ok(c) || c.math != 0) return HEXGNN_EINVAL;
    QPlan qp;
    int rc = make_qplan(c.n, c.b, c.c_in, c.hidden, c.total_layers, &qp);
    if (rc != HEXGNN_OK) return rc;
    if (!c.workspace || c.workspace_bytes < qp.ws_total) return HEXGNN_EWORKSPACE;
    const bool packed = !c.wl && !c.bl && !c.wr;      // (packed by hexgnn_csr_build_grouped_pack of this step)
    if (!c.gptr || (!packed && (!c.wl || !c.bl || !c.wr)) || !c.lin_w || !c.lin_b || !c.v0_w || !c.v0_b || !c.v1_w || !c.v1_b ||
        !c.wpack || !c.saved || !c.status || !c.rowptr || !c.col || !c.rowptr_t || !c.col_t || !c.invdeg || !c.x || !c.acts ||
        !c.q || c.x_stride < c.c_in)
        return HEXGNN_EINVAL;
    rc = launch_pack(qp.sp, c.c_in, c.hidden, c.wl, c.bl, c.wr, c.wpack, st, 0, nullptr);
    if (rc != HEXGNN_OK) return rc;
    QStepArgs a;
    fill_qfwd_args(a.f, c, qp);
    fill_qbwd_args(a.b, c, qp);
    a.b.dq = c.td_dq;
    if (g_prof_class >= 0) {
        // a profile class is being timed: the two launches, so that the per-kernel figures keep their meaning
        {
            KernelTimer kt(HEXGNN_K_QNET_FWD, st);
            rc = launch_qfwd_math(qp.sp.nt, 0, a.f, st);
        }
        if (rc != HEXGNN_OK) return rc;
        KernelTimer kt(HEXGNN_K_QNET_BWD, st);
        rc = launch_qbwd_math(qp.sp.nt, 0, a.b, st);
    } else {
        rc = launch_qstep(qp.sp.nt, a, st);
    }
    if (rc != HEXGNN_OK) return rc;
    return check_launch();
}

// Gradient destinations per layer, and the head tail's in the order (lin_w, lin_b, v0_w, v0_b, v1_w, v1_b).  QGradArrays: how
// the positional entry points name them (HOST pointer arrays); the descriptor names them as flat + offsets.
struct QGrads { float* wl[kMaxLayers]; float* bl[kMaxLayers]; float* wr[kMaxLayers]; float* tail[6]; };
struct QGradArrays { float* const* d_wl; float* const* d_bl; float* const* d_wr; float* tail[6]; };

// the one place where either form becomes per-layer pointers (total_layers is in 1 .. kMaxLayers: make_qplan has passed)
static int resolve_grads(const hexgnn_qnet_call& c, const QGradArrays* arr, QGrads& g) {
    const int L = c.total_layers;
    if (arr) {
        if (!arr->d_wl || !arr->d_bl || !arr->d_wr) return HEXGNN_EINVAL;
        for (int l = 0; l < L; ++l) { g.wl[l] = arr->d_wl[l]; g.bl[l] = arr->d_bl[l]; g.wr[l] = arr->d_wr[l]; }
        for (int k = 0; k < 6; ++k) g.tail[k] = arr->tail[k];
    } else {      // (flat and offsets: checked by hexgnn_qnet_call_backward)
        for (int l = 0; l < L; ++l) {
            g.wl[l] = c.flat + c.offsets[3 * l]; g.bl[l] = c.flat + c.offsets[3 * l + 1]; g.wr[l] = c.flat + c.offsets[3 * l + 2];
        }
        const int64_t* t = c.offsets + 3 * L;
        for (int k = 0; k < 6; ++k) g.tail[k] = (k < 2 || c.mode != 2) ? c.flat + t[k] : nullptr;      // (mode 2: no value head)
    }
    for (int l = 0; l < L; ++l) if (!g.wl[l] || !g.bl[l] || !g.wr[l]) return HEXGNN_EINVAL;
    return HEXGNN_OK;
}

static int qnet_backward_staged_impl(const hexgnn_qnet_call& c, const QGradArrays* arr, int stages, int layer_lo, int layer_hi,
                                     hipStream_t st) {
    const int n = c.n, b = c.b, c_in = c.c_in, hidden = c.hidden, total_layers = c.total_layers, mode = c.mode, math = c.math;
    if (n < 0 || b < 0 || mode < 0 || mode > 2 || math < 0 || math > 1 || c.body_layers < 1 || c.body_layers > total_layers)
        return HEXGNN_EINVAL;
    if (stages <= 0 || (stages & ~(HEXGNN_QBWD_DATA | HEXGNN_QBWD_SMALL | HEXGNN_QBWD_HIDDEN))) return HEXGNN_EINVAL;
    if ((stages & HEXGNN_QBWD_HIDDEN) && (layer_lo < 1 || layer_hi < layer_lo || layer_hi > total_layers)) return HEXGNN_EINVAL;
    const bool st_data = stages & HEXGNN_QBWD_DATA, st_small = stages & HEXGNN_QBWD_SMALL, st_hidden = stages & HEXGNN_QBWD_HIDDEN;
    QPlan qp;
    int rc = make_qplan(n, b, c_in, hidden, total_layers, &qp);
    if (rc != HEXGNN_OK) return rc;
    if (!c.workspace || c.workspace_bytes < qp.ws_total) return HEXGNN_EWORKSPACE;
    QGrads g;
    rc = resolve_grads(c, arr, g);
    if (rc != HEXGNN_OK) return rc;
    float* const* d_wl = g.wl; float* const* d_bl = g.bl; float* const* d_wr = g.wr;
    float *d_lin_w = g.tail[0], *d_lin_b = g.tail[1], *d_v0_w = g.tail[2], *d_v0_b = g.tail[3], *d_v1_w = g.tail[4], *d_v1_b = g.tail[5];
    if (!c.gptr || !c.wpack || !c.saved || !c.lin_w || !d_lin_w || !d_lin_b || !c.status) return HEXGNN_EINVAL;
    if (mode != 2 && (!c.v0_w || !c.v1_w || !d_v0_w || !d_v0_b || !d_v1_w || !d_v1_b)) return HEXGNN_EINVAL;
    if (mode == 1 && !c.d_out_v) return HEXGNN_EINVAL;
    if (n > 0 && (!c.rowptr_t || !c.col_t || !c.invdeg || !c.x || !c.acts || !c.dq)) return HEXGNN_EINVAL;
    const char* sv = (const char*)c.saved;
    const char* hsv = sv + qp.head_saved_off;
    float* part = (float*)((char*)c.workspace + qp.ws_part_off);
    float* part0 = (float*)((char*)c.workspace + qp.ws_part0_off);
    QBwdArgs a;
    fill_qbwd_args(a, c, qp);
    if (b > 0 && n > 0) {
        if (st_data) {
            KernelTimer kt(HEXGNN_K_QNET_BWD, st);
            rc = launch_qbwd_math(qp.sp.nt, math, a, st);
            if (rc != HEXGNN_OK) return rc;
        }
    } else if (st_data) {
        for (int l = 0; l < total_layers; ++l) {
            const int in = (l == 0) ? c_in : hidden;
            (void)hipMemsetAsync(d_wl[l], 0, sizeof(float) * (size_t)hidden * in, st);
            (void)hipMemsetAsync(d_wr[l], 0, sizeof(float) * (size_t)hidden * in, st);
            (void)hipMemsetAsync(d_bl[l], 0, sizeof(float) * (size_t)hidden, st);
        }
        (void)hipMemsetAsync(a.lin_part, 0, sizeof(float) * (size_t)(b > 0 ? b : 1) * (qp.sp.hp + 1), st);
        (void)hipMemsetAsync(a.dz, 0, sizeof(float) * (size_t)(b > 0 ? b : 1) * (hidden / 2), st);
        (void)hipMemsetAsync(a.dvr, 0, sizeof(float) * (size_t)(b > 0 ? b : 1), st);
    }
    if (n > 0 && b > 0) {
        // hidden layers [lo, hi) of this call: weight-gradient GEMM into the stage's own slab region, then ONE reduce launch
        // whose block roles cover those slabs (R0) and -- with HEXGNN_QBWD_SMALL -- the per-graph partials (R1..R3)
        const int lo = st_hidden ? layer_lo : 1, hi = st_hidden ? layer_hi : 1;
        const int nh = hi - lo;
        const size_t slab_sz = (size_t)qp.sp.hp * (2 * qp.sp.hp + 1);
        float* spart = part + (size_t)(lo - 1) * kDwMaxSlices * slab_sz;
        if (nh > 0) {
            rc = launch_weight_grads(n, c_in, hidden, qp.sp, qp.bp, c.x, c.x_stride, c.acts, sv, a.G, d_wl, d_bl, d_wr, spart,
                                     part0, st, math, (const unsigned*)(sv + qp.xmax_off), a.gmax,
                                     /*hidden_only_no_reduce=*/true, lo, hi, c.n_live);
            if (rc != HEXGNN_OK) return rc;
        }
        GradReduceArgs r;
        for (int i = 0; i < nh; ++i) { r.dwl[i] = d_wl[lo + i]; r.dbl[i] = d_bl[lo + i]; r.dwr[i] = d_wr[lo + i]; }
        r.part = spart; r.S = dw_slices_for(n, nh, math, qp.sp.L - (qp.sp.small_first ? 1 : 0)); r.hp = qp.sp.hp; r.H = hidden; r.nh = nh;
        {   // one thread per float4 of a slab; blocks per layer so that all layers together make ~512 equal blocks
            const int q_all = qp.sp.hp * (2 * qp.sp.hp + 1) / 4;
            int bpl = (q_all + 255) / 256;
            if (nh > 0 && bpl * nh < 512) bpl = (512 + nh - 1) / nh;
            if (bpl > (q_all + 31) / 32) bpl = (q_all + 31) / 32;
            r.blk_per_layer = bpl;
            r.per = (q_all + bpl - 1) / bpl;
        }
        r.first_part = a.first_part; r.b = b; r.c_in = c_in; r.dwl0 = d_wl[0]; r.dbl0 = d_bl[0]; r.dwr0 = d_wr[0];
        r.lin_part = a.lin_part; r.d_lin_w = d_lin_w; r.d_lin_b = d_lin_b;
        r.dz = a.dz; r.dvr = a.dvr; r.pooled = (const float*)(hsv + qp.hs.pooled_off); r.z = (const float*)(hsv + qp.hs.z_off);
        r.d_v0_w = d_v0_w; r.d_v0_b = d_v0_b; r.d_v1_w = d_v1_w; r.d_v1_b = d_v1_b;
        r.n0 = nh * r.blk_per_layer;
        r.n1 = st_small ? (hidden * (2 * c_in + 1) + 3) / 4 : 0;
        r.n2 = st_small ? (hidden + 1 + 3) / 4 : 0;
        r.nbx3 = (4 * hidden + 15) / 16;
        r.n3 = (st_small && mode != 2 && hidden / 2 > 0) ? r.nbx3 * (hidden / 2) : 0;
        r.loss_part = c.td_loss ? c.td_loss_part : nullptr; r.loss = c.td_loss;
        const int n4 = (st_small && r.loss_part && r.loss) ? 1 : 0;      // (the block behind the last role: the TD loss's mean)
        if (r.n0 + r.n1 + r.n2 + r.n3 + n4 > 0) qnet_grad_reduce_kernel<<<r.n0 + r.n1 + r.n2 + r.n3 + n4, 256, 0, st>>>(r);
    } else if (st_small) {
        launch_head_param_grads(b, hidden, mode, a.dz, a.dvr, (const float*)(hsv + qp.hs.pooled_off),
                                (const float*)(hsv + qp.hs.z_off), a.lin_part, d_lin_w, d_lin_b, d_v0_w, d_v0_b, d_v1_w,
                                d_v1_b, st);
    }
    return check_launch();
}

extern "C" {

int hexgnn_qnet_supported(int c_in, int hidden, int max_nodes_per_graph) {
    const int hp = padded_width(hidden);
    return hp > 0 && hp <= 112 && hidden >= 2 && c_in >= 1 && c_in <= kSmallCin && c_in != hidden &&
           max_nodes_per_graph <= kRows;
}

int hexgnn_qnet_csr_capacity(int hidden) {
    const int hp = padded_width(hidden);
    if (hp <= 0 || hp > 112 || hidden < 2) return HEXGNN_EUNSUPPORTED;
    HEXGNN_NT_SWITCH7(hp / 16, return QLds<NT_>::col_cap);
    return HEXGNN_EUNSUPPORTED;
}

size_t hexgnn_qnet_saved_bytes(int n, int b, int c_in, int hidden, int total_layers) {
    QPlan q;
    if (n < 0 || b < 0 || make_qplan(n, b, c_in, hidden, total_layers, &q) != HEXGNN_OK) return 0;
    return q.saved_total;
}

size_t hexgnn_qnet_backward_workspace_bytes(int n, int b, int c_in, int hidden, int total_layers) {
    QPlan q;
    if (n < 0 || b < 0 || make_qplan(n, b, c_in, hidden, total_layers, &q) != HEXGNN_OK) return 0;
    return q.ws_total;
}

int hexgnn_qnet_call_forward(const hexgnn_qnet_call* c, int chain_backward, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_qnet_call)) return HEXGNN_EINVAL;
    return chain_backward ? qnet_step_impl(*c, (hipStream_t)stream_) : qnet_forward_impl(*c, (hipStream_t)stream_);
}

int hexgnn_qnet_call_backward(const hexgnn_qnet_call* c, int stages, int layer_lo, int layer_hi, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_qnet_call)) return HEXGNN_EINVAL;
    if (!c->flat || !c->offsets || c->total_layers < 1 || c->total_layers > kMaxLayers) return HEXGNN_EINVAL;
    if (c->td_loss && (!c->td_loss_part || c->mode != 0)) return HEXGNN_EINVAL;
    if (c->n_live) {
        if (!c->td_loss || c->math < 0 || c->math > 1) return HEXGNN_EINVAL;
        if (c->math == 1) return HEXGNN_EUNSUPPORTED;      // (the split-f16 GEMM walks rows by the host's count)
    }
    return qnet_backward_staged_impl(*c, nullptr, stages, layer_lo, layer_hi, (hipStream_t)stream_);
}

// ---- the positional forms: adapters that fill a descriptor ----
int hexgnn_qnet_forward(int n, int b, int c_in, int hidden, int total_layers, int mode, const int* gptr,
                        const int* rowptr, const int* col, const float* invdeg, const float* x, int x_stride,
                        const float* const* wl, const float* const* bl, const float* const* wr,
                        const float* lin_w, const float* lin_b, const float* v0_w, const float* v0_b,
                        const float* v1_w, const float* v1_b, void* wpack, float* acts, void* saved,
                        int need_backward, int acts_layer, int math, float* q, float* out_v, int* status,
                        hexgnn_stream_t stream_) {
    hexgnn_qnet_call c = {};
    c.struct_bytes = sizeof c;
    c.n = n; c.b = b; c.c_in = c_in; c.hidden = hidden; c.total_layers = total_layers; c.mode = mode; c.math = math;
    c.x_stride = x_stride; c.need_backward = need_backward; c.acts_layer = acts_layer;
    c.gptr = gptr; c.rowptr = rowptr; c.col = col; c.invdeg = invdeg; c.x = x;
    c.wl = wl; c.bl = bl; c.wr = wr;
    c.lin_w = lin_w; c.lin_b = lin_b; c.v0_w = v0_w; c.v0_b = v0_b; c.v1_w = v1_w; c.v1_b = v1_b;
    c.wpack = wpack; c.acts = acts; c.saved = saved;
    c.q = q; c.out_v = out_v; c.status = status;
    return qnet_forward_impl(c, (hipStream_t)stream_);
}

int hexgnn_qnet_backward_staged(int n, int b, int c_in, int hidden, int total_layers, int body_layers, int mode, int math,
                                const int* gptr, const int* rowptr_t, const int* col_t, const float* invdeg,
                                const float* x, int x_stride, const float* acts, const void* saved, const void* wpack,
                                const float* lin_w, const float* v0_w, const float* v1_w, const float* dq,
                                const float* d_out_v, float* d_embeds, float* const* d_wl, float* const* d_bl,
                                float* const* d_wr, float* d_lin_w, float* d_lin_b, float* d_v0_w, float* d_v0_b,
                                float* d_v1_w, float* d_v1_b, void* workspace, size_t workspace_bytes, int* status,
                                int stages, int layer_lo, int layer_hi, hexgnn_stream_t stream_) {
    hexgnn_qnet_call c = {};
    c.struct_bytes = sizeof c;
    c.n = n; c.b = b; c.c_in = c_in; c.hidden = hidden; c.total_layers = total_layers; c.body_layers = body_layers;
    c.mode = mode; c.math = math; c.x_stride = x_stride;
    c.gptr = gptr; c.rowptr_t = rowptr_t; c.col_t = col_t; c.invdeg = invdeg; c.x = x;
    c.lin_w = lin_w; c.v0_w = v0_w; c.v1_w = v1_w;
    c.wpack = const_cast<void*>(wpack); c.acts = const_cast<float*>(acts); c.saved = const_cast<void*>(saved);
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.status = status;
    c.dq = dq; c.d_out_v = d_out_v; c.d_embeds = d_embeds;
    const QGradArrays arr = {d_wl, d_bl, d_wr, {d_lin_w, d_lin_b, d_v0_w, d_v0_b, d_v1_w, d_v1_b}};
    return qnet_backward_staged_impl(c, &arr, stages, layer_lo, layer_hi, (hipStream_t)stream_);
}

int hexgnn_qnet_backward(int n, int b, int c_in, int hidden, int total_layers, int body_layers, int mode, int math,
                         const int* gptr, const int* rowptr_t, const int* col_t, const float* invdeg,
                         const float* x, int x_stride, const float* acts, const void* saved, const void* wpack,
                         const float* lin_w, const float* v0_w, const float* v1_w, const float* dq,
                         const float* d_out_v, float* d_embeds, float* const* d_wl, float* const* d_bl,
                         float* const* d_wr, float* d_lin_w, float* d_lin_b, float* d_v0_w, float* d_v0_b,
                         float* d_v1_w, float* d_v1_b, void* workspace, size_t workspace_bytes, int* status,
                         hexgnn_stream_t stream_) {
    return hexgnn_qnet_backward_staged(n, b, c_in, hidden, total_layers, body_layers, mode, math, gptr, rowptr_t, col_t,
                                       invdeg, x, x_stride, acts, saved, wpack, lin_w, v0_w, v1_w, dq, d_out_v, d_embeds,
                                       d_wl, d_bl, d_wr, d_lin_w, d_lin_b, d_v0_w, d_v0_b, d_v1_w, d_v1_b, workspace,
                                       workspace_bytes, status, HEXGNN_QBWD_DATA | HEXGNN_QBWD_SMALL | HEXGNN_QBWD_HIDDEN,
                                       1, total_layers, stream_);
}

#ifdef HEXGNN_STAMPS
// profiling builds only: copies the s_memtime stamps of the exact-fp32 fused kernels to `out` (host pointer)
int hexgnn_debug_stamps(unsigned long long* out, int capacity) {
    const int total = 2 * (kMaxLayers + 2) * kStampPoints * 8;
    if (capacity < total) return HEXGNN_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return HEXGNN_EHIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hexgnn::g_qstamps), sizeof(unsigned long long) * total) != hipSuccess) return HEXGNN_EHIP;
    return total;
}
#endif
}  // extern "C"
