// Row gradients (include/kge_hip_rows.h): coalesce the (id, gradient row) pairs of a row-gradient backward, and update
// only the parameter rows that have a gradient -- the training step that never holds an (n_rows, d) gradient.
//
// kge_rows_coalesce
//   1  kge_key_sort: the stable ascending order `perm` of the ids                                    (key_sort.hip)
//   2  run_heads_kernel: head[j] = 1 where the j-th sorted id differs from the one before it
//   3  mask_scan_launch: per block of 1024 sorted positions, the number of heads before it           (mask_scan.h)
//   4  run_ranks_kernel: rank = heads up to and including j, minus one -- the id's index among the distinct ids.  It goes
//      to rank[perm[j]] (the ORIGINAL position), a head writes uniq[rank] = its id, the last position writes *count
//   5  zero_rows_kernel: the rows [0, *count) of `out`
//   6  kge_segment_sum_ordered with the ranks as keys and the same `perm`        (segment_sum_ordered.hip, shared as is)
// The ordered reduction compares keys for equality and for >= 0 only: under `perm` the ranks have the run boundaries
// of the ids, so what it adds, and in which order, is what it adds for the ids themselves -- into row rank instead of
// row id.  Both start from a zero row: the same bits.
//
// kge_row_sgd / kge_row_adagrad / kge_row_adam: one wavefront per row uniq[j], j < *count read on the device, float4
// accesses when every row starts on 16 bytes and d is a multiple of 4, scalar otherwise.  Pure bandwidth: each touched
// row of the parameter and of its state is read once and written once.  uniq is duplicate-free: one writer per row, no
// atomic.  -ffp-contract=off: the arithmetic is the source's, operation by operation.
#include "kge_common.h"
#include "mask_scan.h"
#include "segment_levels.h"
#include "../../include/kge_hip_det.h"
#include "../../include/kge_hip_rows.h"

namespace {

constexpr int ROW_MAX_BLOCKS = 2048;            // of 4 wavefronts: the grid cap of the row kernels
constexpr int ROW_MAX_WAVES = ROW_MAX_BLOCKS * 4;
constexpr int SEG_MAX_D = 1024;                 // widest row of one kge_segment_sum_ordered call
constexpr int64_t ROWS_MAX_M = 0x7fffffffll;    // kge_key_sort's limit (32-bit positions)

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct CoalesceWs {         // byte offsets into the workspace
    size_t perm, rank, head, scan, sort, sort_bytes, seg, seg_bytes, total;
};

CoalesceWs coalesce_ws(int64_t M, int d)
{
    CoalesceWs w{};
    if (M <= 0 || M > ROWS_MAX_M || d < 1) return w;
    const int dc = d < SEG_MAX_D ? d : SEG_MAX_D;
    size_t off = 0;
    w.perm = off; off += up256((size_t)M * 8);
    w.rank = off; off += up256((size_t)M * 8);
    w.head = off; off += up256((size_t)M);
    w.scan = off; off += up256((size_t)mask_scan_ws_elems(M) * 4);
    // (the sort's size query walks rocPRIM's host-side configuration: remembered for the last M, one training's every step)
    static thread_local int64_t sort_m = 0, sort_bytes = 0;
    if (sort_m != M) { sort_bytes = kge_key_sort_ws_bytes(M, 32); sort_m = M; }
    w.sort = off; w.sort_bytes = (size_t)sort_bytes; off += up256(w.sort_bytes);
    w.seg = off; w.seg_bytes = kge_det_make_plan(M, dc).bytes; off += up256(w.seg_bytes);
    w.total = off;
    return w;
}

__global__ __launch_bounds__(256) void run_heads_kernel(const int64_t *__restrict__ ids, const int64_t *__restrict__ perm,
                                                        int64_t M, uint8_t *__restrict__ head)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x)
        head[j] = j == 0 || ids[perm[j]] != ids[perm[j - 1]];
}

// MS_CT threads over mask_scan_blocks(M) blocks (mask_scan.h: thread t of block b owns b * MS_CB + t * MS_CE + [0, MS_CE))
__global__ __launch_bounds__(MS_CT) void run_ranks_kernel(const int64_t *__restrict__ ids, const int64_t *__restrict__ perm,
                                                          const uint8_t *__restrict__ head,
                                                          const int32_t *__restrict__ block_base, int64_t M,
                                                          int64_t *__restrict__ rank, int64_t *__restrict__ uniq,
                                                          int64_t *__restrict__ count)
{
    int m[MS_CE];
    int heads = mask_thread_prefix(head, M, block_base, m);
    const int64_t j0 = (int64_t)blockIdx.x * MS_CB + threadIdx.x * MS_CE;
#pragma unroll
    for (int e = 0; e < MS_CE; ++e) {
        const int64_t j = j0 + e;
        if (j >= M) break;
        heads += m[e];                          // heads among the sorted positions 0 .. j: at least one (position 0)
        const int64_t at = perm[j];
        rank[at] = heads - 1;
        if (m[e]) uniq[heads - 1] = ids[at];
        if (j == M - 1) *count = heads;
    }
}

__global__ __launch_bounds__(256) void zero_rows_kernel(float *__restrict__ out, int64_t out_ld, int d,
                                                        const int64_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = *count;
    for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += (int64_t)gridDim.x * 4) {
        float *o = out + j * out_ld;
        for (int k = lane; k < d; k += 64) o[k] = 0.f;
    }
}

inline int row_grid(int64_t M)
{
    const int64_t blocks = (M + 3) / 4;
    return (int)(blocks < ROW_MAX_BLOCKS ? blocks : ROW_MAX_BLOCKS);
}

// ---- the updates ----------------------------------------------------------------------------------------------------
enum { OP_SGD = 0, OP_ADAGRAD = 1, OP_ADAM = 2 };

struct RowUpdate {
    float *p, *s0, *s1;         // parameter; Adagrad: sum; Adam: exp_avg, exp_avg_sq
    int64_t p_ld;
    int d;
    const int64_t *uniq, *count;
    const float *g;
    int64_t g_ld;
    float lr, eps, om1, om2;    // lr: the step size as it multiplies the direction
};

template <int OP>
__device__ __forceinline__ void update_one(const RowUpdate &u, float g, float &p, float &a, float &b)
{
    if (OP == OP_SGD) {
        p = p - u.lr * g;
    } else if (OP == OP_ADAGRAD) {
        a = a + g * g;
        p = p - u.lr * (g / (sqrtf(a) + u.eps));
    } else {
        a = a + (g - a) * u.om1;
        b = b + (g * g - b) * u.om2;
        p = p - u.lr * (a / (sqrtf(b) + u.eps));
    }
}

template <int OP, bool VEC>
__global__ __launch_bounds__(256) void row_update_kernel(const RowUpdate u)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = *u.count;
    for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += (int64_t)gridDim.x * 4) {
        const int64_t row = u.uniq[j] * u.p_ld;
        const float *g = u.g + j * u.g_ld;
        if (VEC) {
            for (int k = 4 * lane; k < u.d; k += 256) {
                const float4 gv = *reinterpret_cast<const float4 *>(g + k);
                float4 pv = *reinterpret_cast<const float4 *>(u.p + row + k), av{}, bv{};
                if (OP >= OP_ADAGRAD) av = *reinterpret_cast<const float4 *>(u.s0 + row + k);
                if (OP == OP_ADAM) bv = *reinterpret_cast<const float4 *>(u.s1 + row + k);
                update_one<OP>(u, gv.x, pv.x, av.x, bv.x);
                update_one<OP>(u, gv.y, pv.y, av.y, bv.y);
                update_one<OP>(u, gv.z, pv.z, av.z, bv.z);
                update_one<OP>(u, gv.w, pv.w, av.w, bv.w);
                *reinterpret_cast<float4 *>(u.p + row + k) = pv;
                if (OP >= OP_ADAGRAD) *reinterpret_cast<float4 *>(u.s0 + row + k) = av;
                if (OP == OP_ADAM) *reinterpret_cast<float4 *>(u.s1 + row + k) = bv;
            }
        } else {
            for (int k = lane; k < u.d; k += 64) {
                float pv = u.p[row + k], av = 0.f, bv = 0.f;
                if (OP >= OP_ADAGRAD) av = u.s0[row + k];
                if (OP == OP_ADAM) bv = u.s1[row + k];
                update_one<OP>(u, g[k], pv, av, bv);
                u.p[row + k] = pv;
                if (OP >= OP_ADAGRAD) u.s0[row + k] = av;
                if (OP == OP_ADAM) u.s1[row + k] = bv;
            }
        }
    }
}

template <int OP>
int launch_update(const RowUpdate &u, int64_t M, kge_stream_t stream)
{
    if (M < 0 || u.d < 1 || u.p_ld < u.d || u.g_ld < u.d) return KGE_EINVAL;
    if (M == 0) return 0;
    if (!u.p || !u.uniq || !u.count || !u.g || (OP >= OP_ADAGRAD && !u.s0) || (OP == OP_ADAM && !u.s1)) return KGE_EINVAL;
    const bool vec = u.d % 4 == 0 && u.p_ld % 4 == 0 && u.g_ld % 4 == 0 && kge_aligned16(u.p) && kge_aligned16(u.g) &&
                     (OP < OP_ADAGRAD || kge_aligned16(u.s0)) && (OP != OP_ADAM || kge_aligned16(u.s1));
    hipStream_t s = kge_s(stream);
    if (vec) hipLaunchKernelGGL((row_update_kernel<OP, true>), dim3(row_grid(M)), dim3(256), 0, s, u);
    else hipLaunchKernelGGL((row_update_kernel<OP, false>), dim3(row_grid(M)), dim3(256), 0, s, u);
    KGE_CHECK_LAUNCH();
    return 0;
}

} // namespace

extern "C" size_t kge_rows_coalesce_ws_bytes(int64_t M, int d)
{
    return coalesce_ws(M, d).total;
}

extern "C" int kge_rows_coalesce(const float *rows, int64_t ld, int d, const int64_t *ids, int64_t M, int64_t n_rows,
                                 int64_t *uniq, float *out, int64_t out_ld, int64_t *count, void *ws, size_t ws_bytes,
                                 kge_stream_t stream)
{
    if (M < 0 || M > ROWS_MAX_M || d < 1 || ld < d || out_ld < d || n_rows < 1 || n_rows > ((int64_t)1 << 32) || !count)
        return KGE_EINVAL;
    hipStream_t s = kge_s(stream);
    if (M == 0) {
        hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
        return e == hipSuccess ? 0 : (int)e;
    }
    if (!rows || !ids || !uniq || !out) return KGE_EINVAL;
    const CoalesceWs w = coalesce_ws(M, d);
    if (w.total == 0 || !ws || !kge_aligned16(ws) || ws_bytes < w.total) return KGE_EINVAL;
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < n_rows) ++bits;
    char *base = static_cast<char *>(ws);
    int64_t *perm = reinterpret_cast<int64_t *>(base + w.perm), *rank = reinterpret_cast<int64_t *>(base + w.rank);
    uint8_t *head = reinterpret_cast<uint8_t *>(base + w.head);
    int32_t *scan = reinterpret_cast<int32_t *>(base + w.scan);
    // the first launch: a refusal (the workspace bound is taken at 32 bits) leaves nothing launched
    int rc = kge_key_sort(ids, M, nullptr, 0, bits, perm, base + w.sort, (int64_t)w.sort_bytes, stream);
    if (rc) return rc;
    const int grid = (int)((M + 255) / 256 < 2048 ? (M + 255) / 256 : 2048);
    hipLaunchKernelGGL(run_heads_kernel, dim3(grid), dim3(256), 0, s, ids, perm, M, head);
    KGE_CHECK_LAUNCH();
    rc = mask_scan_launch(head, M, scan, s);
    if (rc) return rc;
    hipLaunchKernelGGL(run_ranks_kernel, dim3((unsigned)mask_scan_blocks(M)), dim3(MS_CT), 0, s, ids, perm, head, scan, M,
                       rank, uniq, count);
    KGE_CHECK_LAUNCH();
    hipLaunchKernelGGL(zero_rows_kernel, dim3(row_grid(M)), dim3(256), 0, s, out, out_ld, d, count);
    KGE_CHECK_LAUNCH();
    for (int c0 = 0; c0 < d; c0 += SEG_MAX_D) {
        const int dc = d - c0 < SEG_MAX_D ? d - c0 : SEG_MAX_D;
        rc = kge_segment_sum_ordered(rows + c0, ld, dc, rank, M, nullptr, 0, perm, out + c0, out_ld, base + w.seg,
                                     w.seg_bytes, stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int kge_row_sgd(float *p, int64_t p_ld, int d, const int64_t *uniq, const int64_t *count, int64_t M,
                           const float *g, int64_t g_ld, float lr, kge_stream_t stream)
{
    RowUpdate u{};
    u.p = p; u.p_ld = p_ld; u.d = d; u.uniq = uniq; u.count = count; u.g = g; u.g_ld = g_ld;
    u.lr = lr;
    return launch_update<OP_SGD>(u, M, stream);
}

extern "C" int kge_row_adagrad(float *p, float *sum, int64_t p_ld, int d, const int64_t *uniq, const int64_t *count,
                               int64_t M, const float *g, int64_t g_ld, float clr, float eps, kge_stream_t stream)
{
    RowUpdate u{};
    u.p = p; u.s0 = sum; u.p_ld = p_ld; u.d = d; u.uniq = uniq; u.count = count; u.g = g; u.g_ld = g_ld;
    u.lr = clr; u.eps = eps;
    return launch_update<OP_ADAGRAD>(u, M, stream);
}

extern "C" int kge_row_adam(float *p, float *exp_avg, float *exp_avg_sq, int64_t p_ld, int d, const int64_t *uniq,
                            const int64_t *count, int64_t M, const float *g, int64_t g_ld, float lr, float om_beta1,
                            float om_beta2, float eps, float bias1, float bias2, kge_stream_t stream)
{
    if (!(bias1 > 0.f) || !(bias2 >= 0.f)) return KGE_EINVAL;
    RowUpdate u{};
    u.p = p; u.s0 = exp_avg; u.s1 = exp_avg_sq; u.p_ld = p_ld; u.d = d; u.uniq = uniq; u.count = count; u.g = g;
    u.g_ld = g_ld;
    u.lr = (float)((double)lr * sqrt((double)bias2) / (double)bias1);
    u.eps = eps; u.om1 = om_beta1; u.om2 = om_beta2;
    return launch_update<OP_ADAM>(u, M, stream);
}

extern "C" int kge_row_update_max_waves(void)
{
    return ROW_MAX_WAVES;
}
