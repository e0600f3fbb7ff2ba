// Split-precision ("f16x3") instantiations of the fused per-graph kernels (kernels: qnet_fused_kernels.h).
#include "qnet_fused_kernels.h"

namespace hexgnn {

int launch_qfwd_split(int nt, const QFwdArgs& a, hipStream_t st) {
    HEXGNN_NT_SWITCH7(nt, (launch_qfwd_m<NT_, 1>(a, st)));
    return HEXGNN_OK;
}
int launch_qbwd_split(int nt, const QBwdArgs& a, hipStream_t st) {
    HEXGNN_NT_SWITCH7(nt, (launch_qbwd_m<NT_, 1>(a, st)));
    return HEXGNN_OK;
}

}  // namespace hexgnn
