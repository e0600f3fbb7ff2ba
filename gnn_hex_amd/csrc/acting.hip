// Acting on Q-values, one wave per graph: epsilon-greedy / argmax action selection and the double-DQN targets, with their C
// entry points.  Both pick "the greedy node" with graph_first_max, and the selection explores with eps_greedy_rank, the pick
// rollout_ply_kernel (env.hip) makes as well (both in hexgnn_reduce.h).
#include "hexgnn_reduce.h"

namespace hexgnn {

// Greedy = first node attaining the maximum of q[gptr[g]+2 : gptr[g+1]] (torch.argmax tie rule;
// GN0/RainbowDQN/evaluate_elo.py:253-266); with u given, env g explores by eps_greedy_rank on its pair u[2g], u[2g+1] (a
// uniformly drawn non-terminal node with probability eps).  Outputs the node rank inside its graph, the vertex id (backmap, what
// Env_manager.validate_actions returns, multi_env_manager.py:62-64) and the exploratory flag.
__global__ __launch_bounds__(64) void select_actions_kernel(int b, const int* __restrict__ gptr, const float* __restrict__ q,
                                                          const int64_t* __restrict__ backmap, float eps,
                                                          const float* __restrict__ u, int* __restrict__ act_vertex,
                                                          int* __restrict__ act_rank, unsigned char* __restrict__ expl) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1];
    float best;
    int arg;
    graph_first_max(q, r0, r1, lane, best, arg);
    if (lane == 0) {
        unsigned char ex;
        const int rank = eps_greedy_rank(arg, r0, r1, eps, u ? u + 2 * g : nullptr, ex);
        act_rank[g] = rank;
        if (act_vertex) act_vertex[g] = rank >= 0 ? (backmap ? (int)backmap[r0 + rank] : rank) : -1;
        if (expl) expl[g] = ex;
    }
}

// double-DQN targets:
//   a2[g] = the greedy node of q_sel in graph g (global index)
//   y[g]  = reward[g] + (gamma_n * q_val[a2[g]]) * (done[g] ? 0 : 1): three separately rounded fp32 operations, the torch
//           expression `r + gamma_n * q_tg[a2] * (~d).float()` bit for bit (an infinite q_val at a done graph gives NaN there too)
// A graph of two or fewer nodes has no non-terminal node: a2[g] = gptr[g] - 1 (rank -1, what hexgnn_select_actions reports)
// and q_val's term is taken as zero, y[g] = reward[g] + (gamma_n * 0) * notdone.
__global__ __launch_bounds__(64) void dqn_targets_kernel(const int* __restrict__ gptr, const float* __restrict__ q_sel,
                                                       const float* __restrict__ q_val, const float* __restrict__ reward,
                                                       const unsigned char* __restrict__ done, float gamma_n,
                                                       float* __restrict__ y, long long* __restrict__ a2) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1];
    float best;
    int arg;
    graph_first_max(q_sel, r0, r1, lane, best, arg);
    if (lane == 0) {
        const bool none = arg == 0x7fffffff;
        const float qv = none ? 0.f : q_val[arg];
        const float notdone = done[g] ? 0.f : 1.f;
        a2[g] = none ? (long long)r0 - 1 : (long long)arg;
        y[g] = __fadd_rn(reward[g], __fmul_rn(__fmul_rn(gamma_n, qv), notdone));
    }
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_select_actions(int b, const int* gptr, const float* q, const int64_t* backmap, float eps, const float* u,
                          int* action_vertex, int* action_rank, uint8_t* exploratory, hexgnn_stream_t stream_) {
    if (b < 0 || (b > 0 && (!gptr || !q || !action_rank))) return HEXGNN_EINVAL;
    if (b == 0) return HEXGNN_OK;
    select_actions_kernel<<<b, 64, 0, (hipStream_t)stream_>>>(b, gptr, q, backmap, eps, u, action_vertex, action_rank,
                                                              exploratory);
    return check_launch();
}

int hexgnn_dqn_targets(int b, const int* gptr, const float* q_sel, const float* q_val, const float* reward,
                       const uint8_t* done, float gamma_n, float* y, int64_t* a2, hexgnn_stream_t stream_) {
    if (b < 0 || (b > 0 && (!gptr || !q_sel || !q_val || !reward || !done || !y || !a2))) return HEXGNN_EINVAL;
    if (b == 0) return HEXGNN_OK;
    dqn_targets_kernel<<<b, 64, 0, (hipStream_t)stream_>>>(gptr, q_sel, q_val, reward, done, gamma_n, y, (long long*)a2);
    return check_launch();
}

}  // extern "C"
