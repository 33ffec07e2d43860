// The fused training criterion (include/kge_hip_train.h): the loss of n (positive, negative) score pairs and its
// closed-form gradients in one pass over the two score vectors, summed in a fixed fp64 tree.
//
// pair_loss_kernel<KIND, GRAD>   G = min(ceil(n / PL_CHUNK), PL_MAX_BLOCKS) blocks of 256 threads; a thread takes 4
//                                consecutive pairs per turn (one 16-byte quad of each vector where its base allows it),
//                                writes their gradients and keeps the sum of their terms in fp64; wavefront butterfly,
//                                LDS across the block's four wavefronts.  G = 1 writes *loss itself.
// st_final_kernel                one block: the G partials of the workspace, added the same way, rounded to fp32 once.
// The tree itself (the turns of a thread, the block sum, the final block), the quad accessors and softplus / sigma are
// loss_common.h, shared with group_loss.hip.
// Pure streaming: 8 bytes read and (GRAD) 8 bytes written per pair; at a training batch (n = 32,768: 0.5 MB) the cost is
// the launches, which is why there are at most two.  -ffp-contract=off: the arithmetic is the source's.
#include "kge_common.h"
#include "../../include/kge_hip_train.h"
#include "loss_common.h"

namespace {

constexpr int PL_THREADS = ST_THREADS;          // the tree of loss_common.h: its blocks, turns and grid cap
constexpr int PL_CHUNK = ST_CHUNK;              // pairs per block and turn
constexpr int PL_MAX_BLOCKS = ST_MAX_BLOCKS;
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

inline int pl_grid(int64_t n) { return st_grid(n); }

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

template <int KIND, bool GRAD>
__global__ __launch_bounds__(PL_THREADS) void pair_loss_kernel(const PairLoss a)
{
    __shared__ double sh[PL_THREADS / 64];
    const double acc = st_thread_sum(a.n, [&](int64_t j, float (&t)[4]) {
        float p[4], q[4], gp[4], gq[4];
        load_quad(a.pos, j, a.n, a.vec & VEC_POS, p);
        load_quad(a.neg, j, a.n, a.vec & VEC_NEG, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = pair_term<KIND>(a.margin, p[e], q[e], gp[e], gq[e]);
        if (GRAD) {
            store_quad(a.dpos, j, a.n, a.vec & VEC_DPOS, gp);
            store_quad(a.dneg, j, a.n, a.vec & VEC_DNEG, gq);
        }
    });
    st_finish_block(acc, sh, a.part, a.loss, a.acc_io);
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
        hipLaunchKernelGGL(st_final_kernel, dim3(1), dim3(ST_THREADS), 0, s, a.part, G, a.loss, a.acc_io);
        KGE_CHECK_LAUNCH();
    }
    return 0;
}
