// The TD loss's per-entry expressions, one copy: the standalone kernels (td_loss.hip) and the fused forward's tail
// (qnet_fused_kernels.h) promise each other's bits.  d = q[sel] - target; loss_fn 0 = squared error, 1 = Huber with delta 1.
// Callers multiply as  w * td_term(d)  and  (gl * w) * td_dterm(d),  gl = grad_loss / k.
#pragma once
#include "hexgnn_common.h"

namespace hexgnn {

__device__ __forceinline__ float td_term(float d, int loss_fn) {
    const float a = fabsf(d);
    return loss_fn == 0 ? d * d : (a <= 1.f ? 0.5f * d * d : a - 0.5f);
}

// d td_term / d d
__device__ __forceinline__ float td_dterm(float d, int loss_fn) {
    return loss_fn == 0 ? 2.f * d : fminf(fmaxf(d, -1.f), 1.f);
}

}  // namespace hexgnn
