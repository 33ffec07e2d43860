// Models whose relation is a linear operator on entity rows: RESCAL and HolE (bilinear_xform.hip), TransR
// (transr_xform.hip).  What their translation units share lives here once:
//   - the relation-grouped transform  out[pos, j] = finish(chain_k x(pos)[k] * C_key(pos)[k][j]),  k ascending, one
//     accumulator per output: rel_query_kernel, parametrised by an Op that says which rows, which operator, which finish;
//   - the pieces of the one-triple-per-wave scoring kernels (normalised row load, grid, the width limit).
// The per-relation outer-product reduction behind kge_rescal_rel_grad / kge_transr_rel_grad is one kernel in
// transr_xform.hip (kge_rel_outer_grad, declared in kge_common.h).
#pragma once
#include "kge_common.h"

namespace {

constexpr int REL_MAXD = 512;   // widest entity / relation row of these models: SC_WAVES rows of it are resident in LDS

// ---- the relation-grouped transform ---------------------------------------------------------------------------------
// A block owns 64 positions of the sorted order (`perm`, or the given order without it) and 64 output columns.  Thread 0
// cuts the 64 rows into runs of equal key; per 16-chunk of k the input rows are staged once (Xs) and the operator tile
// once per RUN (Bs): with the rows sorted by relation a tile of C is read once per group of up to 64 rows instead of once
// per row.  A row accumulates only inside its own run, so its chain is k ascending over its own operator whatever the
// rest of the tile holds: the result depends on (row, key) only, not on the batch, the order or the tile position.
constexpr int QT_ROWS = 64;     // rows of one tile (sorted positions)
constexpr int QT_COLS = 64;     // output columns of one tile
constexpr int QT_KC = 16;       // k chunk staged in LDS
constexpr int QT_THREADS = 256;
constexpr int QT_PER_THREAD = QT_ROWS * QT_COLS / QT_THREADS;   // 16 accumulators

struct RelRow {
    int64_t out = -1;   // output row
    int64_t key = -1;   // rows of one run share it, and with it one operator
    int64_t src = -1;   // row of X, < 0: the row reads as zeros
    float sgn = 0.f;    // for Op::finish
};

struct RelQueryIO {
    const float *X; int64_t ldx;
    const int64_t *perm;            // optional: the positions in key order
    int64_t n_rows;
    float *out; int64_t ldo;
};

// An Op supplies
//   int K, J                                   inner and output width
//   RelRow row(int64_t pos)                    the descriptor of position pos
//   Coefs coefs(int64_t key)                   the operator of a run, resolved once per run (asked per staged element the
//                                              relation's base pointer leaves the scalar registers: +5 % on RESCAL / HolE):
//       bool Coefs::k_contiguous()                 for one j the k lie side by side in memory (else, for one k, the j):
//                                                  the staging loop walks the index that keeps global reads contiguous
//       float Coefs::operator()(int k, int j)      C[k][j]
//   float finish(const RelRow &, int j, float acc)
// FULL: K % QT_KC == 0, the inner loop runs unrolled over whole chunks.
template <class Op, bool FULL>
__global__ __launch_bounds__(QT_THREADS) void rel_query_kernel(const RelQueryIO io, const Op op)
{
    __shared__ float Xs[QT_ROWS][QT_KC + 1];
    __shared__ float Bs[QT_KC][QT_COLS + 1];
    __shared__ int64_t row_out[QT_ROWS], row_key[QT_ROWS], row_src[QT_ROWS];
    __shared__ float row_sgn[QT_ROWS];
    __shared__ int run_lo[QT_ROWS + 1];
    __shared__ int n_runs;
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * QT_ROWS;
    const int nr = (int)((io.n_rows - p0) < QT_ROWS ? (io.n_rows - p0) : QT_ROWS);
    const int c0 = blockIdx.y * QT_COLS;
    const int K = op.K, J = op.J;
    if (tid < QT_ROWS) {
        RelRow w;
        if (tid < nr) w = op.row(io.perm ? io.perm[p0 + tid] : p0 + tid);
        row_out[tid] = w.out; row_key[tid] = w.key; row_src[tid] = w.src; row_sgn[tid] = w.sgn;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < nr; ++i)
            if (i == 0 || row_key[i] != row_key[i - 1]) run_lo[n++] = i;
        run_lo[n] = nr;
        n_runs = n;
    }
    __syncthreads();
    const int col = tid & (QT_COLS - 1), rg = tid / QT_COLS;
    float acc[QT_PER_THREAD];
#pragma unroll
    for (int s = 0; s < QT_PER_THREAD; ++s) acc[s] = 0.f;
    for (int k0 = 0; k0 < K; k0 += QT_KC) {
        const int kn = FULL ? QT_KC : (K - k0 < QT_KC ? K - k0 : QT_KC);
        for (int idx = tid; idx < QT_ROWS * QT_KC; idx += QT_THREADS) {
            const int rr = idx / QT_KC, kk = idx % QT_KC;
            const int64_t src = row_src[rr];
            Xs[rr][kk] = (src >= 0 && kk < kn) ? io.X[src * io.ldx + k0 + kk] : 0.f;
        }
        for (int ru = 0; ru < n_runs; ++ru) {
            const int rs = run_lo[ru], re = run_lo[ru + 1];
            const auto C = op.coefs(row_key[rs]);
            __syncthreads();        // Xs complete; the previous run's readers of Bs are done
            for (int idx = tid; idx < QT_KC * QT_COLS; idx += QT_THREADS) {
                int kk, jj;
                if (C.k_contiguous()) { kk = idx % QT_KC; jj = idx / QT_KC; }
                else { jj = idx % QT_COLS; kk = idx / QT_COLS; }
                const int j = c0 + jj;
                Bs[kk][jj] = (kk < kn && j < J) ? C(k0 + kk, j) : 0.f;
            }
            __syncthreads();
            if (FULL) {
#pragma unroll
                for (int kk = 0; kk < QT_KC; ++kk) {
                    const float b = Bs[kk][col];
#pragma unroll
                    for (int s = 0; s < QT_PER_THREAD; ++s) {
                        const int row = rg + 4 * s;
                        if (row >= rs && row < re) acc[s] = fmaf(Xs[row][kk], b, acc[s]);
                    }
                }
            } else {
                for (int kk = 0; kk < kn; ++kk) {
                    const float b = Bs[kk][col];
#pragma unroll
                    for (int s = 0; s < QT_PER_THREAD; ++s) {
                        const int row = rg + 4 * s;
                        if (row >= rs && row < re) acc[s] = fmaf(Xs[row][kk], b, acc[s]);
                    }
                }
            }
        }
        __syncthreads();            // before the next chunk overwrites Xs
    }
    const int j = c0 + col;
    if (j < J) {
#pragma unroll
        for (int s = 0; s < QT_PER_THREAD; ++s) {
            const int row = rg + 4 * s;
            if (row < nr) {
                const RelRow w{row_out[row], row_key[row], row_src[row], row_sgn[row]};
                io.out[w.out * io.ldo + j] = op.finish(w, j, acc[s]);
            }
        }
    }
}

// ---- scoring_function: one triple per wave, SC_WAVES triples per block ----------------------------------------------
constexpr int SC_WAVES = 4;

// xs = x / max(||x||, 1e-12); returns the clamped norm
__device__ __forceinline__ float load_normalized(const float *__restrict__ x, int d, int lane, float *xs)
{
    float ss = 0.f;
    for (int k = lane; k < d; k += 64) ss = fmaf(x[k], x[k], ss);
    const float n = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    for (int k = lane; k < d; k += 64) xs[k] = x[k] / n;
    return n;
}

inline int sc_grid(int64_t B)
{
    const int64_t blocks = (B + SC_WAVES - 1) / SC_WAVES;
    return (int)(blocks < 8192 ? (blocks > 0 ? blocks : 1) : 8192);
}

} // namespace
