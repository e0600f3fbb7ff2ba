// Match play: the selection of a node per graph by argmax, uniform draw or a draw from softmax(q / T), one wave per graph.
// graph_pick (hexgnn_reduce.h) is the one copy of that selection; the ply kernel of a match (env.hip: arena_ply_kernel, next to
// the game code it plays with) calls the same function, so a pick made here and a move played there agree bit for bit.
#include "hexgnn_reduce.h"

namespace hexgnn {

__global__ __launch_bounds__(64) void sample_actions_kernel(const int* __restrict__ gptr, const float* __restrict__ q,
                                                          const int64_t* __restrict__ backmap, int mode, float temperature,
                                                          const float* __restrict__ u, int* __restrict__ act_vertex,
                                                          int* __restrict__ act_rank, int* __restrict__ status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1];
    bool bad;
    const int rank = graph_pick(q, r0, r1, lane, mode, temperature, u ? u[g] : 0.f, bad);
    if (lane == 0) {
        act_rank[g] = rank;
        if (act_vertex) act_vertex[g] = rank >= 0 ? (backmap ? (int)backmap[r0 + rank] : rank) : -1;
        if (bad && status) atomicOr(status, 1);
    }
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_sample_actions(int b, const int* gptr, const float* q, const int64_t* backmap, int mode, float temperature,
                          const float* u, int* action_vertex, int* action_rank, int* status, hexgnn_stream_t stream_) {
    if (b < 0 || mode < HEXGNN_PICK_GREEDY || mode > HEXGNN_PICK_SOFTMAX) return HEXGNN_EINVAL;
    if (mode == HEXGNN_PICK_SOFTMAX && !(temperature > 0.f && temperature < INFINITY)) return HEXGNN_EINVAL;
    if (b > 0 && (!gptr || !action_rank || (!q && mode != HEXGNN_PICK_UNIFORM) || (!u && mode != HEXGNN_PICK_GREEDY)))
        return HEXGNN_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    if (status) {
        const hipError_t e = hipMemsetAsync(status, 0, sizeof(int), st);
        if (e != hipSuccess) { g_last_hip_error = (int)e; return HEXGNN_EHIP; }
    }
    if (b == 0) return HEXGNN_OK;
    sample_actions_kernel<<<b, 64, 0, st>>>(gptr, q, backmap, mode, temperature, u, action_vertex, action_rank, status);
    return check_launch();
}

}  // extern "C"
