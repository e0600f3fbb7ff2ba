// The one-launch TD step (qnet_step_kernel: forward, TD loss and the backward's data chain of a graph per workgroup), exact fp32
// only.  A translation unit of its own: co-compiled template variants perturb each other's register allocation.
#include "qnet_fused_kernels.h"

namespace hexgnn {

template <int NT>
static int launch_qstep_m(const QStepArgs& a, hipStream_t st) {
    static bool once = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qnet_step_kernel<NT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, QLds<NT>::total);
        return true;
    }();
    (void)once;
    qnet_step_kernel<NT><<<a.f.b, 512, QLds<NT>::total, st>>>(a);
    return HEXGNN_OK;
}

int launch_qstep(int nt, const QStepArgs& a, hipStream_t st) {
    switch (nt) {
        case 1: return launch_qstep_m<1>(a, st);
        case 2: return launch_qstep_m<2>(a, st);
        case 3: return launch_qstep_m<3>(a, st);
        case 4: return launch_qstep_m<4>(a, st);
        case 5: return launch_qstep_m<5>(a, st);
        case 6: return launch_qstep_m<6>(a, st);
        case 7: return launch_qstep_m<7>(a, st);
        default: return HEXGNN_EUNSUPPORTED;
    }
}

}  // namespace hexgnn

#ifdef HEXGNN_STAMPS
// profiling builds only: the s_memtime stamps of qnet_step_kernel (this translation unit's own copy of the stamp array; both
// bodies write it, rows [0] and [1] as the two kernels do) to `out` (host pointer)
extern "C" int hexgnn_debug_stamps_step(unsigned long long* out, int capacity) {
    const int total = 2 * (hexgnn::kMaxLayers + 2) * hexgnn::kStampPoints * 8;
    if (capacity < total) return HEXGNN_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return HEXGNN_EHIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hexgnn::g_qstamps), sizeof(unsigned long long) * total) != hipSuccess) return HEXGNN_EHIP;
    return total;
}
#endif
