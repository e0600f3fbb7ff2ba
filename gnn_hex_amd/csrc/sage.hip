// GraphSAGE stack for gfx950: fused (CSR mean-gather -> fp32 MFMA [agg|x]*[Wl;Wr]^T -> bias -> ReLU) per
// layer, its data-gradient twin, and a batched weight-gradient GEMM.
//
// Reference semantics: CachifiedGNN.forward (GN0/models.py:261-294) over pyg SAGEConv
// (GN0/torch_script_models.py:52-73):  y_i = W_l mean_{j in N(i)} x_j + b_l + W_r x_i ; ReLU every layer.
//
// Data layout (HBM): every node-feature matrix is [n][HP] fp32, HP = 16*NT (pads zero).  A workgroup is
// 8 waves; wave w owns the 16-row block 8*blockIdx+w.  The whole packed weight matrix of the layer
// (2*NT*NT KiB) is staged once per workgroup into LDS in MFMA-fragment order, so every B fragment is one
// conflict-free ds_read_b128.  The A operand never touches LDS: lane (r = l&15, g = l>>4) gathers, for
// its row r, the feature chunks {16c+4g .. 16c+4g+3} of every in-neighbour straight into registers; these
// four floats are the k-slices of four consecutive v_mfma_f32_16x16x4_f32 (the K order is permuted
// consistently on the packed-weight side).  fp32 in / fp32 accumulate: exact fmaf chains, deterministic.
//
// This unit holds the C entry points of the stack: argument checks, the plan, and calls into the units that own the kernels
// (sage_pack.hip, sage_layer.hip, sage_stack.hip, sage_dw.hip).
#include "sage_internal.h"

using namespace hexgnn;

// a block table is usable when it can be a partition of [0, n) into at most kStackFlagWords pieces of at most 128 rows (its
// CONTENT is device data: checked by the kernel, block by block)
static bool block_table_ok(int n, const int* block_starts, int num_blocks) {
    if (!block_starts) return num_blocks == 0;
    // (more blocks than rows is fine: a table built on the device has the block budget's entries whatever n is, the unused ones
    // == n -- empty blocks, which leave at once)
    return num_blocks >= (n + 127) / 128 && num_blocks >= 1 && num_blocks <= kStackFlagWords;
}

// groups of a block table (hexgnn_sage_stack_call.group_starts): a HOST list of block indices, checked here before anything else runs:
// 0 = group_starts[0] < group_starts[1] < ... < group_starts[num_groups] = num_blocks <= kStackFlagWords, over a table
static bool block_groups_ok(const int* block_starts, int num_blocks, const int* group_starts, int num_groups) {
    if (num_groups == 0) return true;
    if (num_groups < 0 || !group_starts || !block_starts || num_blocks < 1 || num_blocks > kStackFlagWords) return false;
    if (group_starts[0] != 0 || group_starts[num_groups] != num_blocks) return false;
    for (int g = 0; g < num_groups; ++g) if (group_starts[g + 1] <= group_starts[g]) return false;
    return true;
}

// the backward workspace of a plan: G (per-layer masked output gradients), the weight-gradient slabs, the raw first layer's partials
struct BwdWs { float *G, *part, *part0; };
static BwdWs carve_workspace(void* workspace, const BwdPlan& b) {
    char* ws = (char*)workspace;
    return {(float*)(ws + b.g_off), (float*)(ws + b.part_off), (float*)(ws + b.part0_off)};
}

// empty batch: all parameter gradients are zero (d_nw / d_nb: the norm stack's, or null)
static void zero_param_grads(int L, int c_in, int hidden, float* const* d_wl, float* const* d_bl, float* const* d_wr,
                             float* const* d_nw, float* const* d_nb, hipStream_t st) {
    for (int l = 0; l < L; ++l) {
        const int in = (l == 0) ? c_in : hidden;
        (void)hipMemsetAsync(d_wl[l], 0, sizeof(float) * (size_t)hidden * in, st);
        (void)hipMemsetAsync(d_wr[l], 0, sizeof(float) * (size_t)hidden * in, st);
        (void)hipMemsetAsync(d_bl[l], 0, sizeof(float) * (size_t)hidden, st);
        if (d_nw) (void)hipMemsetAsync(d_nw[l], 0, sizeof(float) * (size_t)hidden, st);
        if (d_nb) (void)hipMemsetAsync(d_nb[l], 0, sizeof(float) * (size_t)hidden, st);
    }
}

extern "C" {

size_t hexgnn_sage_stack_pack_bytes(int c_in, int hidden, int num_layers) {
    if (hidden > 16 * kMaxNT) { WidePlan w; return wide_make_plan(0, c_in, hidden, num_layers, &w) == HEXGNN_OK ? w.pack_bytes : 0; }
    StackPlan p;
    if (make_plan(0, c_in, hidden, num_layers, &p) != HEXGNN_OK) return 0;
    return p.pack_bytes;
}

size_t hexgnn_sage_stack_saved_bytes(int n, int c_in, int hidden, int num_layers) {
    if (hidden > 16 * kMaxNT) { WidePlan w; return (n >= 0 && wide_make_plan(n, c_in, hidden, num_layers, &w) == HEXGNN_OK) ? w.saved_bytes : 0; }
    StackPlan p;
    if (n < 0 || make_plan(n, c_in, hidden, num_layers, &p) != HEXGNN_OK) return 0;
    return p.saved_bytes;
}

// the descriptor fields the four positional adapters share
static hexgnn_sage_stack_call positional_call(int n, int c_in, int hidden, int num_layers, const int* rowptr_t, const int* col_t,
                                              const float* invdeg, const float* x, int x_stride, const void* wpack,
                                              const float* acts, const void* saved) {
    hexgnn_sage_stack_call c{};
    c.struct_bytes = sizeof c;
    c.n = n; c.c_in = c_in; c.hidden = hidden; c.num_layers = num_layers; c.x_stride = x_stride;
    c.rowptr_t = rowptr_t; c.col_t = col_t; c.invdeg = invdeg; c.x = x;
    c.wpack = const_cast<void*>(wpack); c.acts = const_cast<float*>(acts); c.saved = const_cast<void*>(saved);
    c.tap_layer = -1;
    return c;
}

int hexgnn_sage_stack_forward(int n, int c_in, int hidden, int num_layers, const int* rowptr, const int* col,
                              const float* invdeg, const float* x, int x_stride, const float* const* wl,
                              const float* const* bl, const float* const* wr, void* wpack, float* acts,
                              void* saved, int need_backward, int flags, hexgnn_stream_t stream_) {
    hexgnn_sage_stack_call c = positional_call(n, c_in, hidden, num_layers, nullptr, nullptr, invdeg, x, x_stride, wpack, acts,
                                               saved);
    c.rowptr = rowptr; c.col = col; c.wl = wl; c.bl = bl; c.wr = wr; c.need_backward = need_backward; c.flags = flags;
    return hexgnn_sage_stack_call_forward(&c, stream_);
}

int hexgnn_sage_stack_call_forward(const hexgnn_sage_stack_call* call, hexgnn_stream_t stream_) {
    if (!call || call->struct_bytes != sizeof(hexgnn_sage_stack_call)) return HEXGNN_EINVAL;
    const hexgnn_sage_stack_call& c = *call;
    hipStream_t st = (hipStream_t)stream_;
    const bool norm = c.nw || c.nb;
    const int n = c.n, flags = c.flags;
    const int* block_starts = c.block_starts;
    int num_blocks = c.num_blocks;
    StackPlan p;
    if (norm && (block_starts || num_blocks || c.group_starts || c.num_groups || flags)) return HEXGNN_EINVAL;
    if (!block_groups_ok(block_starts, num_blocks, c.group_starts, c.num_groups)) return HEXGNN_EINVAL;
    if (n < 0 || (flags & ~HEXGNN_SAGE_LINEAR_LAST)) return HEXGNN_EINVAL;
    if (n > 0 && !block_table_ok(n, block_starts, num_blocks)) return HEXGNN_EINVAL;
    if (norm && c.n_live && c.need_backward) return HEXGNN_EINVAL;       // a live row count is an acting-time (forward-only) notion
    if (!norm && c.hidden > 16 * kMaxNT) {   // 129..256: the plain kernels of wide.hip (always materialise the aggregates in `saved`)
        if (!c.wl || !c.bl || !c.wr || !c.wpack) return HEXGNN_EINVAL;
        if (n > 0 && (!c.rowptr || !c.col || !c.invdeg || !c.x || !c.acts)) return HEXGNN_EINVAL;
        return wide_stack_forward(n, c.c_in, c.hidden, c.num_layers, c.rowptr, c.col, c.invdeg, c.x, c.x_stride, c.wl, c.bl, c.wr,
                                  c.wpack, c.acts, c.saved, flags, st);
    }
    int rc = make_plan(n, c.c_in, c.hidden, c.num_layers, &p);
    if (rc != HEXGNN_OK) return rc;
    // (the plain stack's three arrays all NULL: packed by the CSR call already)
    if (!c.wpack || ((!c.wl || !c.bl || !c.wr) && (norm || c.wl || c.bl || c.wr))) return HEXGNN_EINVAL;
    if (norm && (!c.nw || !c.nb || !c.stats || !c.norm_ws)) return HEXGNN_EINVAL;
    if (n > 0 && (!c.rowptr || !c.col || !c.invdeg || !c.x || !c.acts || (norm && !c.pre))) return HEXGNN_EINVAL;
    if (c.need_backward && !c.saved) return HEXGNN_EINVAL;
    if (p.small_first ? c.x_stride < c.c_in : c.x_stride != p.hp) return HEXGNN_EINVAL;
    for (int l = 0; norm && l < p.L; ++l) if (!c.nw[l] || !c.nb[l]) return HEXGNN_EINVAL;

    rc = launch_pack(p, c.c_in, c.hidden, c.wl, c.bl, c.wr, c.wpack, st, 0);
    if (rc != HEXGNN_OK) return rc;
    if (n == 0) return check_launch();

    const size_t slab = (size_t)n * p.hp;
    char* wp = (char*)c.wpack;
    char* sv = (char*)c.saved;
    const int fh = p.small_first ? 1 : 0;
    if (norm) {     // a launch per layer into `pre`, each followed by its norm + ReLU into `acts`
        for (int l = 0; l < p.L; ++l) {
            float* y = c.pre + slab * l;
            const float* bias = (const float*)(wp + p.bias_off[l]);
            float* agg = c.need_backward ? (float*)(sv + p.agg_off[l]) : nullptr;
            if (l == 0 && p.small_first) {
                launch_first_fwd(n, c.c_in, p.hp, c.rowptr, c.col, c.invdeg, c.x, c.x_stride, (const float*)(wp + p.fwd_off[0]), bias, y, agg, 0, st);
            } else {
                rc = launch_layer_fwd(p.nt, n, c.rowptr, c.col, c.invdeg, l == 0 ? c.x : c.acts + slab * (l - 1), wp + p.fwd_off[l], bias,
                                      y, agg, 0, st);
                if (rc != HEXGNN_OK) return rc;
            }
            rc = hexgnn_graph_layernorm_forward_live(n, c.n_live, c.hidden, y, c.nw[l], c.nb[l], c.eps, 1, c.acts + slab * l,
                                                     c.stats + 2 * l, c.norm_ws, c.norm_ws_bytes, stream_);
            if (rc != HEXGNN_OK) return rc;
        }
        return check_launch();
    }
    rc = stack_status(true);
    if (rc != HEXGNN_OK) return rc;
    // groups whose largest fits the resident-workgroup budget run one launch each; otherwise they are ignored
    const bool grouped = c.num_groups > 0 && stack_groups_fit(n, c.group_starts, c.num_groups, p.nt, p.L - fh, st, false);
    const bool one_launch = grouped || choose_stack_launch(n, &block_starts, &num_blocks, p.nt, p.L - fh, st, false);
    // the raw first layer, then all hidden layers in one launch (per group) or a launch per layer
    for (int l = 0; l < p.L; ++l) {
        float* y = c.acts + slab * l;
        const float* bias = (const float*)(wp + p.bias_off[l]);
        float* agg = c.need_backward ? (float*)(sv + p.agg_off[l]) : nullptr;
        const int relu = !(l == p.L - 1 && (flags & HEXGNN_SAGE_LINEAR_LAST));
        if (l == 0 && p.small_first) {
            launch_first_fwd(n, c.c_in, p.hp, c.rowptr, c.col, c.invdeg, c.x, c.x_stride, (const float*)(wp + p.fwd_off[0]), bias, y, agg, relu, st);
        } else if (one_launch) {
            StackKArgs a{};
            a.n = n; a.l_first = l; a.n_layers = p.L - l;
            a.relu_last = !(flags & HEXGNN_SAGE_LINEAR_LAST); a.last_of_stack = p.L - 1; a.tap_layer = -1;
            a.rowptr = c.rowptr; a.col = c.col; a.invdeg = c.invdeg;
            a.in0 = l == 0 ? c.x : c.acts + slab * (l - 1);
            a.slabs = c.acts; a.slab = slab;
            a.w0 = wp + p.fwd_off[l]; a.wstride = p.L - l > 1 ? p.fwd_off[l + 1] - p.fwd_off[l] : 0;
            a.b0 = wp + p.bias_off[l];
            a.agg0 = c.need_backward ? sv + p.agg_off[l] : nullptr;
            a.astride = p.L - l > 1 ? p.agg_off[l + 1] - p.agg_off[l] : 0;
            a.flags = reinterpret_cast<unsigned*>(wp + p.flag_off);
            a.bstart = block_starts; a.nblocks = num_blocks;
            for (int g = 0; g < (grouped ? c.num_groups : 1) && rc == HEXGNN_OK; ++g) {
                if (grouped) { a.gbase = c.group_starts[g]; a.gcount = c.group_starts[g + 1] - c.group_starts[g]; }
                rc = launch_stack(false, p.nt, a, st, !grouped || g + 1 == c.num_groups);
            }
            if (rc != HEXGNN_OK) return rc;
            break;
        } else {
            const float* xin = l == 0 ? c.x : c.acts + slab * (l - 1);
            rc = launch_layer_fwd(p.nt, n, c.rowptr, c.col, c.invdeg, xin, wp + p.fwd_off[l], bias, y, agg, relu, st);
            if (rc != HEXGNN_OK) return rc;
        }
    }
    return check_launch();
}

size_t hexgnn_sage_stack_backward_workspace_bytes(int n, int c_in, int hidden, int num_layers) {
    if (hidden > 16 * kMaxNT) { WidePlan w; return (n >= 0 && wide_make_plan(n, c_in, hidden, num_layers, &w) == HEXGNN_OK) ? w.bwd_bytes : 0; }
    StackPlan p;
    if (n < 0 || make_plan(n, c_in, hidden, num_layers, &p) != HEXGNN_OK) return 0;
    BwdPlan b;
    make_bwd_plan(n, p, &b);
    return b.total;
}

int hexgnn_sage_stack_backward(int n, int c_in, int hidden, int num_layers, const int* rowptr, const int* col,
                               const int* rowptr_t, const int* col_t, const float* invdeg, const float* x,
                               int x_stride, const float* acts, const void* saved, const void* wpack,
                               const float* dy, float* dx, float* const* d_wl, float* const* d_bl,
                               float* const* d_wr, void* workspace, size_t workspace_bytes, int flags,
                               hexgnn_stream_t stream_) {
    hexgnn_sage_stack_call c = positional_call(n, c_in, hidden, num_layers, rowptr_t, col_t, invdeg, x, x_stride, wpack, acts,
                                               saved);
    c.rowptr = rowptr; c.col = col; c.flags = flags;
    c.dy = dy; c.dx = dx; c.d_wl = d_wl; c.d_bl = d_bl; c.d_wr = d_wr; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return hexgnn_sage_stack_call_backward(&c, stream_);
}

// data-gradient chain of the plain stack, top layer first: G_{L-1} = dy * [y_{L-1} > 0], then per hidden-input layer l one launch
//   G_{l-1} = ( [ sum_{T} G_l / deg | G_l ] [W_l ; W_r] ) * [y_{l-1} > 0]      (l == 0: the stack-input gradient dx, unmasked)
static int plain_backward_chain(const hexgnn_sage_stack_call& c, const StackPlan& p, float* G, hipStream_t st) {
    const int n = c.n;
    const size_t slab = (size_t)n * p.hp;
    const char* wp = (const char*)c.wpack;
    const int* block_starts = c.block_starts;
    int num_blocks = c.num_blocks;
    const int first_hidden = p.small_first ? 1 : 0;
    if (c.flags & HEXGNN_SAGE_DY_IN_PLACE) {
        // the caller's producer (hexgnn_head_backward with HEXGNN_HEAD_MASK_DH) wrote G_{L-1} = dy * [y_{L-1} > 0] straight
        // into its slab of the workspace: nothing to combine
        if (c.dy != G + slab * (p.L - 1)) return HEXGNN_EINVAL;
    } else {
        const bool relu_top = !(c.flags & HEXGNN_SAGE_LINEAR_LAST);
        launch_combine(n, p.hp, c.rowptr_t, c.col_t, c.dy, nullptr, relu_top ? c.acts + slab * (p.L - 1) : nullptr,
                       G + slab * (p.L - 1), st);
    }
    int rc = stack_status(true);
    if (rc != HEXGNN_OK) return rc;
    const int lo = (first_hidden == 0 && !c.dx) ? 1 : first_hidden;        // last layer whose data gradient is wanted
    const bool grouped = c.num_groups > 0 && stack_groups_fit(n, c.group_starts, c.num_groups, p.nt, p.L - lo, st, true);
    const bool one_launch = grouped || choose_stack_launch(n, &block_starts, &num_blocks, p.nt, p.L - lo, st, true);
    if (one_launch) {
        StackKArgs a{};
        a.n = n; a.l_first = p.L - 1; a.n_layers = p.L - lo;
        a.tap_layer = c.tap_out ? c.tap_layer : -1; a.tap_out = c.tap_out;
        a.rowptr = c.rowptr_t; a.col = c.col_t; a.invdeg = c.invdeg;
        a.in0 = G + slab * (p.L - 1);
        a.slabs = G; a.slab = slab; a.masks = c.acts; a.dx = c.dx;
        a.w0 = wp + p.bwd_off[p.L - 1]; a.wstride = p.bwd_off[p.L - 1] - p.bwd_off[p.L - 2];
        a.flags = reinterpret_cast<unsigned*>(const_cast<char*>(wp) + p.flag_off) + kStackFlagWords;
        a.bstart = block_starts; a.nblocks = num_blocks;
        for (int g = 0; g < (grouped ? c.num_groups : 1) && rc == HEXGNN_OK; ++g) {
            if (grouped) { a.gbase = c.group_starts[g]; a.gcount = c.group_starts[g + 1] - c.group_starts[g]; }
            rc = launch_stack(true, p.nt, a, st, !grouped || g + 1 == c.num_groups);
        }
        return rc;
    }
    for (int l = p.L - 1; l >= first_hidden; --l) {
        float* out = l >= 1 ? G + slab * (l - 1) : c.dx;
        if (!out) break;                                   // l == 0 and nobody asked for the input gradient
        const float* ymask = l >= 1 ? c.acts + slab * (l - 1) : nullptr;
        // (the gradient w.r.t. layer tap_layer's OUTPUT, before its ReLU mask, leaves the same launch: the epilogue stores
        // the rows twice)
        float* tap = (c.tap_out && l - 1 == c.tap_layer) ? c.tap_out : nullptr;
        rc = launch_layer_bwd(p.nt, n, c.rowptr_t, c.col_t, c.invdeg, G + slab * l, wp + p.bwd_off[l], ymask, out, tap, st);
        if (rc != HEXGNN_OK) return rc;
    }
    return HEXGNN_OK;
}

// ... of the norm stack, top layer first: norm backward (mask by the layer's output, d gamma / d beta) gives G_l = gradient at the
// contraction's output; the layer kernel turns it into the gradient at the layer's input = the next norm's dy (one scratch slab)
static int norm_backward_chain(const hexgnn_sage_stack_call& c, const StackPlan& p, float* G, float* tmp, hexgnn_stream_t stream_) {
    const size_t slab = (size_t)c.n * p.hp;
    const char* wp = (const char*)c.wpack;
    const int first_hidden = p.small_first ? 1 : 0;
    const float* dcur = c.dy;
    for (int l = p.L - 1; l >= 0; --l) {
        int rc = hexgnn_graph_layernorm_backward(c.n, c.hidden, c.pre + slab * l, c.acts + slab * l, c.nw[l], c.stats + 2 * l, dcur,
                                                 c.eps, 1, G + slab * l, c.d_nw[l], c.d_nb[l], c.norm_ws, c.norm_ws_bytes, stream_);
        if (rc != HEXGNN_OK) return rc;
        if (l < first_hidden) break;
        float* out = l >= 1 ? tmp : c.dx;
        if (!out) break;
        rc = launch_layer_bwd(p.nt, c.n, c.rowptr_t, c.col_t, c.invdeg, G + slab * l, wp + p.bwd_off[l], nullptr, out, nullptr,
                              (hipStream_t)stream_);
        if (rc != HEXGNN_OK) return rc;
        dcur = tmp;
    }
    return HEXGNN_OK;
}

int hexgnn_sage_stack_call_backward(const hexgnn_sage_stack_call* call, hexgnn_stream_t stream_) {
    if (!call || call->struct_bytes != sizeof(hexgnn_sage_stack_call)) return HEXGNN_EINVAL;
    const hexgnn_sage_stack_call& c = *call;
    hipStream_t st = (hipStream_t)stream_;
    const bool norm = c.nw || c.nb;
    const int n = c.n, flags = c.flags;
    StackPlan p;
    if (norm && (c.block_starts || c.num_blocks || c.group_starts || c.num_groups || c.tap_out || flags)) return HEXGNN_EINVAL;
    if (!block_groups_ok(c.block_starts, c.num_blocks, c.group_starts, c.num_groups)) return HEXGNN_EINVAL;
    if (n < 0 || (flags & ~(HEXGNN_SAGE_LINEAR_LAST | HEXGNN_SAGE_DY_IN_PLACE))) return HEXGNN_EINVAL;
    if (n > 0 && !block_table_ok(n, c.block_starts, c.num_blocks)) return HEXGNN_EINVAL;
    if ((flags & HEXGNN_SAGE_DY_IN_PLACE) && (flags & HEXGNN_SAGE_LINEAR_LAST)) return HEXGNN_EINVAL;
    if (!norm && c.hidden > 16 * kMaxNT) {
        if (!c.d_wl || !c.d_bl || !c.d_wr || !c.wpack || !c.saved) return HEXGNN_EINVAL;
        if (n > 0 && (!c.rowptr_t || !c.col_t || !c.invdeg || !c.x || !c.acts || !c.dy)) return HEXGNN_EINVAL;
        return wide_stack_backward(n, c.c_in, c.hidden, c.num_layers, c.rowptr_t, c.col_t, c.invdeg, c.x, c.x_stride, c.acts,
                                   c.saved, c.wpack, c.dy, c.dx, c.d_wl, c.d_bl, c.d_wr, c.workspace, c.workspace_bytes, flags,
                                   c.tap_layer, c.tap_out, st);
    }
    int rc = make_plan(n, c.c_in, c.hidden, c.num_layers, &p);
    if (rc != HEXGNN_OK) return rc;
    BwdPlan b;
    make_bwd_plan(n, p, &b);
    // (the norm stack: + one scratch slab behind the plain stack's workspace)
    const size_t need = b.total + (norm ? align_up(sizeof(float) * (size_t)n * p.hp, 256) : 0);
    if (!c.workspace || c.workspace_bytes < need) return HEXGNN_EWORKSPACE;
    if (!c.d_wl || !c.d_bl || !c.d_wr || !c.wpack || !c.saved) return HEXGNN_EINVAL;
    if (norm && (!c.d_nw || !c.d_nb || !c.nw || !c.stats || !c.norm_ws)) return HEXGNN_EINVAL;
    for (int l = 0; l < p.L; ++l) {
        if (!c.d_wl[l] || !c.d_bl[l] || !c.d_wr[l]) return HEXGNN_EINVAL;
        if (norm && (!c.d_nw[l] || !c.d_nb[l] || !c.nw[l])) return HEXGNN_EINVAL;
    }
    if (n > 0 && (!c.rowptr_t || !c.col_t || !c.invdeg || !c.x || !c.acts || !c.dy || (norm && !c.pre))) return HEXGNN_EINVAL;
    if (n > 0 && c.tap_out && (c.tap_layer < 0 || c.tap_layer >= p.L - 1)) return HEXGNN_EINVAL;

    const BwdWs w = carve_workspace(c.workspace, b);
    if (n == 0) {
        zero_param_grads(p.L, c.c_in, c.hidden, c.d_wl, c.d_bl, c.d_wr, norm ? c.d_nw : nullptr, norm ? c.d_nb : nullptr, st);
        return check_launch();
    }
    rc = norm ? norm_backward_chain(c, p, w.G, (float*)((char*)c.workspace + b.total), stream_)
              : plain_backward_chain(c, p, w.G, st);
    if (rc != HEXGNN_OK) return rc;
    rc = launch_weight_grads(n, c.c_in, c.hidden, p, b, c.x, c.x_stride, c.acts, (const char*)c.saved, w.G, c.d_wl, c.d_bl, c.d_wr,
                             w.part, w.part0, st);
    if (rc != HEXGNN_OK) return rc;
    return check_launch();
}

/* ---- SAGE stack with the whole-batch LayerNorm of --norm=True between every contraction and its ReLU ------------------------
 * (CachifiedGNN.forward with norms, GN0/models.py:261-294: conv -> norm -> relu per layer).  One call per direction instead of
 * a SAGE call + a norm call per layer: the weights are packed once, and the weight gradients of all layers are ONE batched
 * GEMM + one reduce (per-layer launches of 64-128 workgroups ran at a quarter of the batched rate).  The same descriptor with
 * nw / nb set; these are its positional adapters. */
size_t hexgnn_sage_norm_stack_backward_workspace_bytes(int n, int c_in, int hidden, int num_layers) {
    StackPlan p;
    if (n < 0 || make_plan(n, c_in, hidden, num_layers, &p) != HEXGNN_OK) return 0;
    BwdPlan b;
    make_bwd_plan(n, p, &b);
    return b.total + align_up(sizeof(float) * (size_t)n * p.hp, 256);
}

int hexgnn_sage_norm_stack_forward(int n, int c_in, int hidden, int num_layers, const int* rowptr, const int* col,
                                   const float* invdeg, const float* x, int x_stride, const float* const* wl,
                                   const float* const* bl, const float* const* wr, const float* const* nw,
                                   const float* const* nb, float eps, void* wpack, float* pre, float* acts, void* saved,
                                   float* stats, void* norm_ws, size_t norm_ws_bytes, int need_backward,
                                   hexgnn_stream_t stream_) {
    if (!nw || !nb) return HEXGNN_EINVAL;        // (without them the descriptor would describe the plain stack)
    hexgnn_sage_stack_call c = positional_call(n, c_in, hidden, num_layers, nullptr, nullptr, invdeg, x, x_stride, wpack, acts,
                                               saved);
    c.rowptr = rowptr; c.col = col; c.wl = wl; c.bl = bl; c.wr = wr; c.need_backward = need_backward;
    c.nw = nw; c.nb = nb; c.eps = eps; c.pre = pre; c.stats = stats; c.norm_ws = norm_ws; c.norm_ws_bytes = norm_ws_bytes;
    return hexgnn_sage_stack_call_forward(&c, stream_);
}

int hexgnn_sage_norm_stack_backward(int n, int c_in, int hidden, int num_layers, const int* rowptr_t, const int* col_t,
                                    const float* invdeg, const float* x, int x_stride, const float* pre,
                                    const float* acts, const void* saved, const void* wpack, const float* stats,
                                    const float* const* nw, float eps, const float* dy, float* dx, float* const* d_wl,
                                    float* const* d_bl, float* const* d_wr, float* const* d_nw, float* const* d_nb,
                                    void* workspace, size_t workspace_bytes, void* norm_ws, size_t norm_ws_bytes,
                                    hexgnn_stream_t stream_) {
    if (!nw) return HEXGNN_EINVAL;               // (without it the descriptor would describe the plain stack)
    hexgnn_sage_stack_call c = positional_call(n, c_in, hidden, num_layers, rowptr_t, col_t, invdeg, x, x_stride, wpack, acts,
                                               saved);
    c.nw = nw; c.eps = eps; c.pre = const_cast<float*>(pre); c.stats = const_cast<float*>(stats);
    c.norm_ws = norm_ws; c.norm_ws_bytes = norm_ws_bytes;
    c.dy = dy; c.dx = dx; c.d_wl = d_wl; c.d_bl = d_bl; c.d_wr = d_wr; c.d_nw = d_nw; c.d_nb = d_nb;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return hexgnn_sage_stack_call_backward(&c, stream_);
}

#ifdef HEXGNN_STAMPS
// profiling builds only: s_memtime stamps of the layer-major kernels' last launches -> `out` (host pointer, 2 x 8 x 8)
int hexgnn_debug_layer_stamps(unsigned long long* out, int capacity) {
    if (capacity < 128) return HEXGNN_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return HEXGNN_EHIP;
    if (read_layer_stamps(out) != HEXGNN_OK) return HEXGNN_EHIP;
    if (capacity >= 384) {       // + the one-launch stack kernels' stamps, [2][16][8]
        if (read_stack_stamps(out + 128) != HEXGNN_OK) return HEXGNN_EHIP;
        return 384;
    }
    return 128;
}
#endif

}  // extern "C"
