// Plan and weight packing of a SAGE stack: the fp32 fragment-order pack of every call and the split-f16 pack of the fused
// kernels (math mode 1).  Used by the stack entry points (sage.hip), the CSR call that packs alongside (csr.hip) and the
// fused path (qnet_fused.hip).
#include "hexgnn_internal.h"
#include "hexgnn_pack.h"

namespace hexgnn {

int make_plan(int n, int c_in, int hidden, int L, StackPlan* p) {
    const int hp = padded_width(hidden);
    if (hp < 0 || L < 1 || L > kMaxLayers) return HEXGNN_EUNSUPPORTED;
    if (c_in != hidden && (c_in < 1 || c_in > kSmallCin)) return HEXGNN_EUNSUPPORTED;
    // rows are addressed through raw-buffer resources with 32-bit byte offsets and num_records 2^31 - 1: a slab of n rows must
    // stay below 2 GiB (4.7 M nodes at hidden 112: ~150x the largest BASELINE batch), beyond it loads would return zeros
    if (n > 0 && (size_t)n * hp * sizeof(float) > 0x7fffffffull) return HEXGNN_EUNSUPPORTED;
    p->hp = hp; p->nt = hp / 16; p->L = L; p->c_in = c_in;
    p->small_first = (c_in != hidden);
    size_t off = 0, soff = 0;
    const size_t pack = (size_t)2 * p->nt * p->nt * 64 * sizeof(f32x4);
    for (int l = 0; l < L; ++l) {
        if (l == 0 && p->small_first) {
            p->fwd_off[l] = off; off += sizeof(float) * (size_t)hp * kSmallCin * 2;  // [HP][8] Wl, [HP][8] Wr
            p->bwd_off[l] = 0;
            p->agg_off[l] = soff; soff += align_up(sizeof(float) * (size_t)n * kSmallCin, 256);
        } else {
            p->fwd_off[l] = off; off += pack;
            p->bwd_off[l] = off; off += pack;
            p->agg_off[l] = soff; soff += align_up(sizeof(float) * (size_t)n * hp, 256);
        }
        p->bias_off[l] = off; off += align_up(sizeof(float) * (hp + 2), 256);   // bias[hp], then {w scale, 1/scale} (math 1)
    }
    p->flag_off = off; off += sizeof(unsigned) * 2 * kStackFlagWords;
    p->pack_bytes = off;
    p->saved_bytes = soff;
    return HEXGNN_OK;
}

// ---- weight packing (one launch per stack call; grid.y = layer): body in hexgnn_pack.h -------------------------------------
__global__ void sage_pack_kernel(PackArgs a, char* __restrict__ wpack) {
    sage_pack_body(a, wpack, blockIdx.x, blockIdx.y, gridDim.x);
}

// ---- split-precision packing for the fused kernels (math mode 1, "f16x3"): every fp32 weight w of a layer is scaled
//      by the layer's power of two s_W (max |w| * s_W in [2^14, 2^15)) and stored as two fp16 planes hi = f16(w s_W),
//      lo = f16(w s_W - hi): 22 significand bits.  The contraction W*X ~= Whi*Xhi + Whi*Xlo + Wlo*Xhi runs on the f16
//      MFMA pipe with fp32 accumulation (rows get their own power-of-two scale in the kernel; both are undone exactly in
//      the epilogue).  Product error ~3*2^-22 relative to max|w| max|x|; measured parity in tests/test_gpu_model.py.
//      Layout per K-half (NT*NT KiB, identical size to the fp32 pack): units u = chunk pairs (2p, 2p+1) [+ one odd
//      chunk]; unit of s chunks at byte (first_chunk*NT) KiB; tile t at + t*s KiB; plane hi at +0, lo at + s*512 B;
//      lane l at + l*8*s B holding the k-slots (kq = l>>4): j < 4 -> feature 16*c0 + 4*kq + j, j >= 4 -> 16*(c0+1) + 4*kq + j-4.
struct Pack16Args {
    LayerPtrs p;
    size_t fwd_off[kMaxLayers], bwd_off[kMaxLayers], bias_off[kMaxLayers];
    int nt, L, hidden, first_hidden, hp;
    unsigned* zero_maxima;    // 2*kMaxLayers words cleared by the scale kernel (per-layer activation / gradient maxima), or null
};
__device__ __forceinline__ unsigned short f16_bits(float v) { _Float16 b = (_Float16)v; return __builtin_bit_cast(unsigned short, b); }
__device__ __forceinline__ float f16_to_f32(unsigned short u) { return (float)__builtin_bit_cast(_Float16, u); }

// per hidden layer: s_W = 2^(14 - floor(log2 max|w|)) over W_l and W_r, stored with its inverse after the padded bias
__global__ __launch_bounds__(1024) void sage_wscale_kernel(Pack16Args a, char* __restrict__ wpack) {
    const int l = a.first_hidden + blockIdx.x;
    const int H = a.hidden;
    const float* wl = a.p.wl[l];
    const float* wr = a.p.wr[l];
    if (blockIdx.x == 0 && a.zero_maxima && threadIdx.x < 2 * kMaxLayers) a.zero_maxima[threadIdx.x] = 0u;
    float m = 0.f;
    for (int i = threadIdx.x; i < H * H; i += 1024) m = fmaxf(m, fmaxf(fabsf(wl[i]), fabsf(wr[i])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float sm[16];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 16; ++w) m = fmaxf(m, sm[w]);
        const unsigned e = __builtin_bit_cast(unsigned, m) >> 23;
        const bool ok = e >= 64u && e <= 190u;
        float* out = reinterpret_cast<float*>(wpack + a.bias_off[l]) + a.hp;
        out[0] = ok ? __builtin_bit_cast(float, (268u - e) << 23) : 1.f;
        out[1] = ok ? __builtin_bit_cast(float, (e - 14u) << 23) : 1.f;
    }
}

__global__ void sage_pack16_kernel(Pack16Args a, char* __restrict__ wpack) {
    const int l = a.first_hidden + blockIdx.y;
    const int nt = a.nt, H = a.hidden;
    const float* wl = a.p.wl[l];
    const float* wr = a.p.wr[l];
    const float wscale = reinterpret_cast<const float*>(wpack + a.bias_off[l])[a.hp];
    // one thread per (direction, half, chunk c, tile t, lane, j<4): 2*2*nt*nt*64*4 elements
    const int per_dir = 2 * nt * nt * 256;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= 2 * per_dir) return;
    const int dir = tid / per_dir;              // 0 forward, 1 backward
    int rem = tid % per_dir;
    const int half = rem / (nt * nt * 256); rem %= nt * nt * 256;
    const int c = rem / (nt * 256); rem %= nt * 256;
    const int t = rem / 256; rem %= 256;
    const int lane = rem >> 2, j = rem & 3;
    const int kq = lane >> 4, m = lane & 15;
    const float* w = half == 0 ? wl : wr;
    float v;
    if (dir == 0) {   // forward: k = input feature 16c+4kq+j, output o = 16t+m
        const int k = 16 * c + 4 * kq + j, o = 16 * t + m;
        v = (k < H && o < H) ? w[o * H + k] : 0.f;
    } else {          // backward: k = output o = 16c+4kq+j, produces input feature i = 16t+m
        const int o = 16 * c + 4 * kq + j, i = 16 * t + m;
        v = (o < H && i < H) ? w[o * H + i] : 0.f;
    }
    v *= wscale;
    const unsigned short hi = f16_bits(v);
    const unsigned short lo = f16_bits(v - f16_to_f32(hi));
    const bool paired = (c | 1) < nt;           // chunk belongs to a full pair
    const int c0 = c & ~1;
    const int s = paired ? 2 : 1;
    const int unit_first = paired ? c0 : c;
    char* base = wpack + (dir == 0 ? a.fwd_off[l] : a.bwd_off[l]) + (size_t)half * nt * nt * 1024
               + (size_t)unit_first * nt * 1024 + (size_t)t * s * 1024;
    const int jj = paired ? (c - c0) * 4 + j : j;
    unsigned short* ph = reinterpret_cast<unsigned short*>(base + lane * 8 * s) + jj;
    unsigned short* pl = reinterpret_cast<unsigned short*>(base + s * 512 + lane * 8 * s) + jj;
    *ph = hi;
    *pl = lo;
}

int fill_pack_args(const StackPlan& p, int c_in, int hidden, const float* const* wl, const float* const* bl,
                   const float* const* wr, PackArgs* pa) {
    for (int l = 0; l < p.L; ++l) {
        if (!wl[l] || !bl[l] || !wr[l]) return HEXGNN_EINVAL;
        pa->p.wl[l] = wl[l]; pa->p.bl[l] = bl[l]; pa->p.wr[l] = wr[l];
        pa->fwd_off[l] = p.fwd_off[l]; pa->bwd_off[l] = p.bwd_off[l]; pa->bias_off[l] = p.bias_off[l];
    }
    pa->hp = p.hp; pa->nt = p.nt; pa->L = p.L; pa->c_in = c_in; pa->hidden = hidden; pa->small_first = p.small_first;
    pa->flag_off = p.flag_off;
    return HEXGNN_OK;
}

int launch_pack(const StackPlan& p, int c_in, int hidden, const float* const* wl, const float* const* bl,
                const float* const* wr, void* wpack, hipStream_t st, int math, unsigned* zero_maxima) {
    if (!wl && !bl && !wr && math == 0) return HEXGNN_OK;      // packed already (hexgnn_csr_build_grouped_pack of this forward)
    if (!wl || !bl || !wr) return HEXGNN_EINVAL;
    PackArgs pa;
    const int rcp = fill_pack_args(p, c_in, hidden, wl, bl, wr, &pa);
    if (rcp != HEXGNN_OK) return rcp;
    const int pack_elems = 2 * p.nt * p.nt * 256;
    sage_pack_kernel<<<dim3((pack_elems + 255) / 256, p.L), 256, 0, st>>>(pa, (char*)wpack);
    if (math == 1) {   // overwrite the hidden layers' weight packs with the split-f16 layout (biases / raw layer stay fp32)
        Pack16Args pb;
        pb.p = pa.p;
        for (int l = 0; l < p.L; ++l) { pb.fwd_off[l] = p.fwd_off[l]; pb.bwd_off[l] = p.bwd_off[l]; pb.bias_off[l] = p.bias_off[l]; }
        pb.nt = p.nt; pb.L = p.L; pb.hidden = hidden; pb.first_hidden = p.small_first ? 1 : 0; pb.hp = p.hp;
        pb.zero_maxima = zero_maxima;
        const int nh = p.L - pb.first_hidden;
        const int elems = 2 * 2 * p.nt * p.nt * 256;
        if (nh > 0) {
            sage_wscale_kernel<<<nh, 1024, 0, st>>>(pb, (char*)wpack);
            sage_pack16_kernel<<<dim3((elems + 255) / 256, nh), 256, 0, st>>>(pb, (char*)wpack);
        }
    }
    return HEXGNN_OK;
}

}  // namespace hexgnn
