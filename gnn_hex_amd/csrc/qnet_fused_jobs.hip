// Several weight sets over one batch in ONE load-balanced forward launch (double-DQN targets: online + target network on the
// next states): the job-table instantiations of the fused forward (kernel body: qnet_fused_kernels.h), the kernel that builds the
// job table and packs the sets' weights, and their C ABI (the targets themselves: hexgnn_dqn_targets, acting.hip).
#include "qnet_fused_kernels.h"
#include "hexgnn_pack.h"

namespace hexgnn {

template <int NT>
static int launch_qfwd_jobs_m(int njobs, const QFwdJobArgs& a, hipStream_t st) {
    static bool once = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qnet_fwd_kernel<NT, 0, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, QLds<NT>::total);
        return true;
    }();
    (void)once;
    qnet_fwd_kernel<NT, 0, true><<<njobs, 512, QLds<NT>::total, st>>>(a);
    return HEXGNN_OK;
}
int launch_qfwd_jobs(int nt, int njobs, const QFwdJobArgs& a, hipStream_t st) {
    HEXGNN_NT_SWITCH7(nt, (launch_qfwd_jobs_m<NT_>(njobs, a, st)));
    return HEXGNN_OK;
}

// ---- job table + weight packs: one launch for up to kPackSets sets (grid.z = set, grid.y = layer; y == L: the table) --------
// The table orders the graphs by DESCENDING node count, ties by ascending graph index (a counting sort over the node counts in
// LDS: deterministic, no host sync), job j = (order[j / k], j % k): the k forwards of one graph are neighbours and share x and
// CSR lines in L2, and the dispatcher -- which hands workgroups out in index order as CUs free up -- runs the longest jobs first.
constexpr int kPackSets = 2;        // sets per launch: 2 x 3 x kMaxLayers pointers fill the 4 KiB of kernel arguments
constexpr int kJobBins = kRows + 2; // node counts 0 .. kRows, and one bin for anything larger (sorted first; the forward poisons it)
struct JobsPackArgs {
    const float* p[kPackSets][3 * kMaxLayers];      // set s: (wl, bl, wr) of layer l at [3 l ..]
    char* wpack[kPackSets];
    size_t fwd0, bias0, fwd1, lstride, bias_rel;    // the plan: layer 0; layer l >= 1 at fwd1 + (l - 1) lstride, bias bias_rel behind
    int hp, nt, L, c_in, hidden, nsets;
    const int* gptr; int b, k; int* jobs;           // jobs == null: packs only
};

__global__ __launch_bounds__(256) void qnet_jobs_pack_kernel(JobsPackArgs a) {
    const int l = blockIdx.y, s = blockIdx.z;
    if (l < a.L) {
        if (s >= a.nsets) return;
        const float* const* p = a.p[s] + 3 * l;
        const size_t fwd = l == 0 ? a.fwd0 : a.fwd1 + (size_t)(l - 1) * a.lstride;
        const size_t bias = l == 0 ? a.bias0 : fwd + a.bias_rel;
        sage_pack_layer(p[0], p[1], p[2], a.wpack[s], fwd, 0, bias, a.hp, a.nt, a.c_in, a.hidden, l == 0,
                        (int)(blockIdx.x * 256 + threadIdx.x), true);
        return;
    }
    if (blockIdx.x != 0 || s != 0 || !a.jobs) return;
    __shared__ int start[kJobBins];
    __shared__ int keys[256];
    const int tid = threadIdx.x, b = a.b, k = a.k;
    auto key_of = [&](int g) { const int c = a.gptr[g + 1] - a.gptr[g]; return c < 0 ? 0 : (c > kRows ? kRows + 1 : c); };
    for (int i = tid; i < kJobBins; i += 256) start[i] = 0;
    __syncthreads();
    for (int g = tid; g < b; g += 256) atomicAdd(&start[key_of(g)], 1);
    __syncthreads();
    if (tid == 0) {      // counts -> first position of every bin, largest count first
        int run = 0;
        for (int c = kJobBins - 1; c >= 0; --c) { const int h = start[c]; start[c] = run; run += h; }
    }
    __syncthreads();
    for (int base = 0; base < b; base += 256) {      // 256 graphs at a time, in graph order: equal counts keep it
        const int g = base + tid;
        const int key = g < b ? key_of(g) : -1;
        keys[tid] = key;
        __syncthreads();
        if (key >= 0) {
            int rank = 0;
            for (int t = 0; t < tid; ++t) rank += keys[t] == key ? 1 : 0;
            const int pos = start[key] + rank;
            for (int w = 0; w < k; ++w) a.jobs[(size_t)pos * k + w] = (g << 2) | w;
        }
        __syncthreads();
        if (key >= 0) atomicAdd(&start[key], 1);
        __syncthreads();
    }
}

}  // namespace hexgnn

using namespace hexgnn;

namespace {
// the plan of the job-table form: the fused path's own (qnet_fused.hip make_qplan), forward side
int jobs_plan(int n, int c_in, int hidden, int L, StackPlan* sp) {
    const int rc = make_plan(n, c_in, hidden, L, sp);
    if (rc != HEXGNN_OK) return rc;
    if (!sp->small_first || sp->nt > 7 || !hexgnn_qnet_supported(c_in, hidden, 0)) return HEXGNN_EUNSUPPORTED;
    return HEXGNN_OK;
}
}  // namespace

extern "C" {

size_t hexgnn_qnet_jobs_bytes(int b, int k) {
    if (b < 0 || k < 1 || k > HEXGNN_MAX_SETS) return 0;
    return sizeof(int) * (size_t)b * k;
}

size_t hexgnn_qnet_multi_workspace_bytes(int n, int b, int c_in, int hidden, int total_layers, int k) {
    StackPlan sp;
    if (n < 0 || b < 0 || k < 1 || k > HEXGNN_MAX_SETS || jobs_plan(n, c_in, hidden, total_layers, &sp) != HEXGNN_OK) return 0;
    return (size_t)k * align_up(sp.pack_bytes, 256) + align_up(hexgnn_qnet_jobs_bytes(b, k), 256);
}

int hexgnn_qnet_forward_jobs(int b, int k, const int* gptr, int* jobs, int c_in, int hidden, int total_layers,
                             const float* const* const* wl, const float* const* const* bl, const float* const* const* wr,
                             void* const* wpack, hexgnn_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (b < 0 || k < 1 || k > HEXGNN_MAX_SETS || !jobs || (b > 0 && !gptr)) return HEXGNN_EINVAL;
    const bool packs = wl || bl || wr || wpack;
    JobsPackArgs a = {};
    a.gptr = gptr; a.b = b; a.k = k; a.jobs = b > 0 ? jobs : nullptr;
    a.L = 0; a.nsets = 0;
    dim3 grid(1, 1, 1);
    if (packs) {
        if (!wl || !bl || !wr || !wpack) return HEXGNN_EINVAL;
        StackPlan sp;
        const int rc = jobs_plan(0, c_in, hidden, total_layers, &sp);
        if (rc != HEXGNN_OK) return rc;
        for (int s = 0; s < k; ++s) {
            if (!wl[s] || !bl[s] || !wr[s] || !wpack[s]) return HEXGNN_EINVAL;
            for (int l = 0; l < sp.L; ++l) if (!wl[s][l] || !bl[s][l] || !wr[s][l]) return HEXGNN_EINVAL;
        }
        a.fwd0 = sp.fwd_off[0]; a.bias0 = sp.bias_off[0];
        a.fwd1 = sp.L > 1 ? sp.fwd_off[1] : 0; a.bias_rel = sp.L > 1 ? sp.bias_off[1] - sp.fwd_off[1] : 0;
        a.lstride = sp.L > 2 ? sp.fwd_off[2] - sp.fwd_off[1] : 0;
        for (int l = 1; l < sp.L; ++l)      // (the kernel recomputes the plan's offsets instead of carrying three tables)
            if (sp.fwd_off[l] != a.fwd1 + (size_t)(l - 1) * a.lstride || sp.bias_off[l] != sp.fwd_off[l] + a.bias_rel)
                return HEXGNN_EUNSUPPORTED;
        a.hp = sp.hp; a.nt = sp.nt; a.L = sp.L; a.c_in = c_in; a.hidden = hidden;
        const int pack_elems = 2 * sp.nt * sp.nt * 256, small_elems = sp.hp * kSmallCin;
        grid.x = ((pack_elems > small_elems ? pack_elems : small_elems) + 255) / 256;
    }
    // the table rides with the first launch; sets beyond kPackSets take a second one
    for (int s0 = 0; s0 < (packs ? k : 1); s0 += kPackSets) {
        if (packs) {
            a.nsets = k - s0 < kPackSets ? k - s0 : kPackSets;
            for (int s = 0; s < a.nsets; ++s) {
                a.wpack[s] = (char*)wpack[s0 + s];
                for (int l = 0; l < a.L; ++l) {
                    a.p[s][3 * l] = wl[s0 + s][l]; a.p[s][3 * l + 1] = bl[s0 + s][l]; a.p[s][3 * l + 2] = wr[s0 + s][l];
                }
            }
            grid.z = a.nsets;
        }
        if (s0 > 0) a.jobs = nullptr;
        if (a.L == 0 && !a.jobs) break;
        grid.y = a.L + 1;
        qnet_jobs_pack_kernel<<<grid, 256, 0, st>>>(a);
    }
    return check_launch();
}

int hexgnn_qnet_forward_multi(int n, int b, int k, int c_in, int hidden, int total_layers, const int* gptr,
                              const int* rowptr, const int* col, const float* invdeg, const float* x, int x_stride,
                              const int* jobs, const void* const* wpack, const float* const* const* tail,
                              float* const* q, int* const* status, hexgnn_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (n < 0 || b < 0 || k < 1 || k > HEXGNN_MAX_SETS) return HEXGNN_EINVAL;
    StackPlan sp;
    const int rc = jobs_plan(n, c_in, hidden, total_layers, &sp);
    if (rc != HEXGNN_OK) return rc;
    if (!jobs || !gptr || !wpack || !tail || !q || !status) return HEXGNN_EINVAL;
    if (n > 0 && (!rowptr || !col || !invdeg || !x)) return HEXGNN_EINVAL;
    if (x_stride < c_in) return HEXGNN_EINVAL;
    QFwdJobArgs a = {};       // (the base's per-set, saved-tensor and TD fields stay null: never read)
    a.jobs = jobs;
    for (int s = 0; s < k; ++s) {
        if (!wpack[s] || !tail[s] || !status[s] || (n > 0 && !q[s])) return HEXGNN_EINVAL;
        for (int j = 0; j < 6; ++j) if (!tail[s][j]) return HEXGNN_EINVAL;
        for (int t = 0; t < s; ++t) if (n > 0 && q[t] == q[s]) return HEXGNN_EINVAL;      // two sets never write the same words
        QSet& e = a.set[s];
        e.wpack = (const char*)wpack[s];
        e.lin_w = tail[s][0]; e.lin_b = tail[s][1]; e.v0_w = tail[s][2]; e.v0_b = tail[s][3]; e.v1_w = tail[s][4]; e.v1_b = tail[s][5];
        e.q = q[s]; e.status = status[s];
    }
    for (int s = k; s < kMaxSets; ++s) a.set[s] = a.set[0];
    if (b == 0 || n == 0) return HEXGNN_OK;
    QFwdArgs& f = a;
    f.n = n; f.b = b; f.c_in = c_in; f.H = hidden; f.L = total_layers; f.mode = 0; f.x_stride = x_stride; f.need_backward = 0;
    f.acts_layer = total_layers;       // (no layer: the job-table form has no activation stores at all)
    f.gptr = gptr; f.rowptr = rowptr; f.col = col; f.invdeg = invdeg; f.x = x;
    for (int l = 0; l < total_layers; ++l) { f.fwd_off[l] = sp.fwd_off[l]; f.bias_off[l] = sp.bias_off[l]; f.agg_off[l] = 0; }
    {
        KernelTimer kt(HEXGNN_K_QNET_FWD, st);
        const int rcl = launch_qfwd_jobs(sp.nt, b * k, a, st);
        if (rcl != HEXGNN_OK) return rcl;
    }
    return check_launch();
}

}  // extern "C"
