// The fused training criterion (include/kge_hip_train.h): the loss of n (positive, negative) score pairs and its
// closed-form gradients in one pass over the two score vectors, summed in a fixed fp64 tree.
//
// pair_loss_kernel<KIND, GRAD>   G = min(ceil(n / PL_CHUNK), PL_MAX_BLOCKS) blocks of 256 threads; a thread takes 4
//                                consecutive pairs per turn (one 16-byte quad of each vector where its base allows it),
//                                writes their gradients and keeps the sum of their terms in fp64; wavefront butterfly,
//                                LDS across the block's four wavefronts.  G = 1 writes *loss itself.
// pair_loss_final_kernel         one block: the G partials of the workspace, added the same way, rounded to fp32 once.
// Pure streaming: 8 bytes read and (GRAD) 8 bytes written per pair; at a training batch (n = 32,768: 0.5 MB) the cost is
// the launches, which is why there are at most two.  -ffp-contract=off: the arithmetic is the source's.
#include "kge_common.h"
#include "../../include/kge_hip_train.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_CHUNK = KGE_PAIR_LOSS_CHUNK;   // pairs per block and turn
constexpr int PL_MAX_BLOCKS = 1024;
constexpr int64_t PL_MAX_N = 0x7fffffffll;
constexpr float BCE_CAP = 100.f;
static_assert(PL_CHUNK == 4 * PL_THREADS, "a thread owns one quad per turn");

enum { VEC_POS = 1, VEC_NEG = 2, VEC_DPOS = 4, VEC_DNEG = 8 };

struct PairLoss {
    const float *pos, *neg;
    float *dpos, *dneg;
    float *loss, *acc_io;
    double *part;
    int64_t n;
    float margin;
    int vec;            // VEC_* bits: which of the four vectors start on 16 bytes
};

inline int pl_grid(int64_t n)
{
    const int64_t g = (n + PL_CHUNK - 1) / PL_CHUNK;
    return (int)(g < PL_MAX_BLOCKS ? g : PL_MAX_BLOCKS);
}

__device__ __forceinline__ void load_quad(const float *__restrict__ x, int64_t j, int64_t n, bool vec, float (&v)[4])
{
    if (vec && j + 4 <= n) {
        const float4 q = *reinterpret_cast<const float4 *>(x + j);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j + e < n ? x[j + e] : 0.f;
    }
}

__device__ __forceinline__ void store_quad(float *__restrict__ x, int64_t j, int64_t n, bool vec, const float (&v)[4])
{
    if (vec && j + 4 <= n) {
        *reinterpret_cast<float4 *>(x + j) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j + e < n) x[j + e] = v[e];
    }
}

// softplus(x) and sigma(x) from one e = exp(-|x|) in (0, 1]: no overflow, no inf / inf
__device__ __forceinline__ void softplus_sigma(float x, float &sp, float &sg)
{
    const float e = expf(-fabsf(x));
    sp = fmaxf(x, 0.f) + log1pf(e);
    const float den = 1.f + e;
    sg = (x >= 0.f ? 1.f : e) / den;
}

template <int KIND>
__device__ __forceinline__ float pair_term(float margin, float p, float q, float &gp, float &gq)
{
    if (KIND == KGE_LOSS_MARGIN) {
        const float a = margin - (p - q);       // MarginLoss's own order: p - q is exact for scores within a factor 2
        const bool on = a >= 0.f;
        gp = on ? -1.f : 0.f;
        gq = on ? 1.f : 0.f;
        return fmaxf(a, 0.f);
    }
    float sp, sq, gsp, gsq;
    softplus_sigma(-p, sp, gsp);        // d softplus(-p) / dp = -sigma(-p)
    softplus_sigma(q, sq, gsq);
    gp = -gsp;
    gq = gsq;
    if (KIND == KGE_LOSS_BCE) {
        if (sp > BCE_CAP) { sp = BCE_CAP; gp = 0.f; }
        if (sq > BCE_CAP) { sq = BCE_CAP; gq = 0.f; }
    }
    return sp + sq;
}

// the 256 fp64 values of a block, in the fixed order of the header; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ void write_loss(const PairLoss &a, double s)
{
    const float l = (float)s;
    *a.loss = l;
    if (a.acc_io) *a.acc_io = *a.acc_io + l;
}

template <int KIND, bool GRAD>
__global__ __launch_bounds__(PL_THREADS) void pair_loss_kernel(const PairLoss a)
{
    __shared__ double sh[PL_THREADS / 64];
    double acc = 0.0;
    const int64_t step = (int64_t)gridDim.x * PL_CHUNK;
    for (int64_t j = (int64_t)blockIdx.x * PL_CHUNK + 4 * threadIdx.x; j < a.n; j += step) {
        float p[4], q[4], gp[4], gq[4], t[4];
        load_quad(a.pos, j, a.n, a.vec & VEC_POS, p);
        load_quad(a.neg, j, a.n, a.vec & VEC_NEG, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float term = pair_term<KIND>(a.margin, p[e], q[e], gp[e], gq[e]);
            t[e] = j + e < a.n ? term : 0.f;
        }
        acc += ((double)t[0] + (double)t[1]) + ((double)t[2] + (double)t[3]);
        if (GRAD) {
            store_quad(a.dpos, j, a.n, a.vec & VEC_DPOS, gp);
            store_quad(a.dneg, j, a.n, a.vec & VEC_DNEG, gq);
        }
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) write_loss(a, s);
        else a.part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(PL_THREADS) void pair_loss_final_kernel(const PairLoss a, int G)
{
    __shared__ double sh[PL_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < G; i += PL_THREADS) acc += a.part[i];
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) write_loss(a, s);
}

template <int KIND>
void launch_stage1(const PairLoss &a, int G, bool grad, hipStream_t s)
{
    if (grad) hipLaunchKernelGGL((pair_loss_kernel<KIND, true>), dim3(G), dim3(PL_THREADS), 0, s, a);
    else hipLaunchKernelGGL((pair_loss_kernel<KIND, false>), dim3(G), dim3(PL_THREADS), 0, s, a);
}

} // namespace

extern "C" size_t kge_pair_loss_ws_bytes(int64_t n)
{
    if (n <= 0 || n > PL_MAX_N) return 0;
    return (size_t)pl_grid(n) * sizeof(double);
}

extern "C" int kge_pair_loss_max_blocks(void)
{
    return PL_MAX_BLOCKS;
}

extern "C" int kge_pair_loss(int kind, float margin, const float *pos, const float *neg, int64_t n, float *loss,
                             float *acc_io, float *dpos, float *dneg, void *ws, size_t ws_bytes, kge_stream_t stream)
{
    if (kind < KGE_LOSS_MARGIN || kind > KGE_LOSS_BCE || n < 0 || n > PL_MAX_N || !loss || (dpos == nullptr) != (dneg == nullptr))
        return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    if (n == 0) {
        hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), s);
        return e == hipSuccess ? 0 : (int)e;
    }
    const size_t need = kge_pair_loss_ws_bytes(n);
    if (!pos || !neg || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) != 0 || ws_bytes < need) return KGE_EINVAL;
    PairLoss a{};
    a.pos = pos; a.neg = neg; a.dpos = dpos; a.dneg = dneg; a.loss = loss; a.acc_io = acc_io;
    a.part = static_cast<double *>(ws);
    a.n = n; a.margin = margin;
    a.vec = (kge_aligned16(pos) ? VEC_POS : 0) | (kge_aligned16(neg) ? VEC_NEG : 0) |
            (dpos && kge_aligned16(dpos) ? VEC_DPOS : 0) | (dneg && kge_aligned16(dneg) ? VEC_DNEG : 0);
    const int G = pl_grid(n);
    const bool grad = dpos != nullptr;
    if (kind == KGE_LOSS_MARGIN) launch_stage1<KGE_LOSS_MARGIN>(a, G, grad, s);
    else if (kind == KGE_LOSS_LOGISTIC) launch_stage1<KGE_LOSS_LOGISTIC>(a, G, grad, s);
    else launch_stage1<KGE_LOSS_BCE>(a, G, grad, s);
    KGE_CHECK_LAUNCH();
    if (G > 1) {
        hipLaunchKernelGGL(pair_loss_final_kernel, dim3(1), dim3(PL_THREADS), 0, s, a, G);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}
