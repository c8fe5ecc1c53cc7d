// encode.hip -- the eval-mode VAE encoder as ONE affine map (pangaea_amd/models/VAENET.py: affine_encoder folds
// Linear / BatchNorm1d(running statistics) / LeakyReLU(slope 1) / Dropout(eval) / l_mu into W_eff, b_eff):
//     out[r, :] = [abd[r, :], tnf[r, :]] . w + b
// pg_affine_rows applies the map to the rows (first half of this file), pg_affine_fold folds one layer into it (second half).
// A translation unit of its own, so that work on it cannot touch the timed kernels' code objects.
//
// The two input matrices are read where they lie (no cat); products and sums are float64 (vector FP64 FMA is full rate on
// CDNA and the kernel is bound by the read of the inputs either way), narrowed to float32 once.  Every output is ONE chain
// of fma over k = 0, 1, .. K-1 starting from b: the order depends neither on the grid nor on n_rows, so a row gives the
// same bits in whichever batch it arrives.
//
// A workgroup of 256 threads owns ROWS = 128 rows and walks K in tiles of KT = 32 inputs.  Per tile the LDS holds the
// float32 rows (128 x 32, rows padded by 16 B: the 16-B reads of four consecutive rows then fall on distinct banks) and the
// float64 slice of w (32 x NOUT, 8 or 16 KB -- never the whole matrix, several workgroups fit a CU).  A thread keeps a
// register tile of 4 rows x NOUT/8 outputs: one 16-B read of a row serves four k, one 16-B read of w two outputs of four
// rows.  The next tile is fetched into registers while the current one is multiplied.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pangaea_feat.h"
#include "pg_internal.h"

namespace {

constexpr int THREADS = 256;
constexpr int ROWS = 128;                 // rows of a workgroup
constexpr int KT = 32;                    // inputs of a tile
constexpr int XLD = KT + 4;               // floats of a row of the tile in LDS
constexpr int TR = 4;                     // rows of a thread: ty, ty + 32, ty + 64, ty + 96
constexpr int XPER = ROWS * KT / THREADS; // floats of the tile a thread fetches
static_assert(KT == 32 && ROWS == TR * (THREADS / 8) && XPER % 4 == 0, "the index arithmetic of fetch / park and the thread tile");

// NOUT: the output width the tile is laid out for (n_out rounded up to 32 or 64; the columns beyond n_out hold zeros and are
// never stored).  VEC: both matrices can be read 16 bytes at a time (row lengths multiples of 4, bases 16-B aligned).
template <int NOUT, bool VEC>
__global__ __launch_bounds__(THREADS) void affine_rows_kernel(const float *__restrict__ abd, int n_abd, const float *__restrict__ tnf, int n_tnf,
                                                              int64_t n_rows, const double *__restrict__ w, const double *__restrict__ b, int n_out,
                                                              float *__restrict__ out)
{
    constexpr int TC = NOUT / 8;          // outputs of a thread: the pairs (j * 8 + tx) * 2, j < TC / 2
    constexpr int WPER = KT * NOUT / THREADS;
    __shared__ __attribute__((aligned(16))) float xs[ROWS * XLD];
    __shared__ __attribute__((aligned(16))) double ws[KT * NOUT];

    const int t = threadIdx.x, tx = t & 7, ty = t >> 3;
    const int K = n_abd + n_tnf;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;

    float xreg[XPER];
    double wreg[WPER];

    // element (row, k) of the concatenated input, zero outside it
    auto fetch = [&](int k0) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < XPER / 4; ++j) {
                const int i = t + THREADS * j, r = i >> 3, k = k0 + (i & 7) * 4;       // (KT / 4 = 8 pieces per row)
                const int64_t row = row0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < n_rows && k < K)                                              // (n_abd % 4 == 0: a piece lies in one matrix)
                    v = k < n_abd ? *reinterpret_cast<const float4 *>(abd + row * n_abd + k)
                                  : *reinterpret_cast<const float4 *>(tnf + row * n_tnf + (k - n_abd));
                xreg[4 * j] = v.x; xreg[4 * j + 1] = v.y; xreg[4 * j + 2] = v.z; xreg[4 * j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < XPER; ++j) {
                const int i = t + THREADS * j, r = i >> 5, k = k0 + (i & 31);
                const int64_t row = row0 + r;
                float v = 0.f;
                if (row < n_rows && k < K) v = k < n_abd ? abd[row * n_abd + k] : tnf[row * n_tnf + (k - n_abd)];
                xreg[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < WPER; ++j) {
            const int i = t + THREADS * j, k = k0 + i / NOUT, o = i % NOUT;
            wreg[j] = (k < K && o < n_out) ? w[(int64_t)k * n_out + o] : 0.0;
        }
    };
    auto park = [&]() {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < XPER / 4; ++j) {
                const int i = t + THREADS * j;
                *reinterpret_cast<float4 *>(&xs[(i >> 3) * XLD + (i & 7) * 4]) = make_float4(xreg[4 * j], xreg[4 * j + 1], xreg[4 * j + 2], xreg[4 * j + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < XPER; ++j) {
                const int i = t + THREADS * j;
                xs[(i >> 5) * XLD + (i & 31)] = xreg[j];
            }
        }
#pragma unroll
        for (int j = 0; j < WPER; ++j) ws[t + THREADS * j] = wreg[j];
    };

    double acc[TR][TC];
#pragma unroll
    for (int j = 0; j < TC / 2; ++j) {
        const int o = (j * 8 + tx) * 2;
        const double b0 = o < n_out ? b[o] : 0.0, b1 = o + 1 < n_out ? b[o + 1] : 0.0;
#pragma unroll
        for (int r = 0; r < TR; ++r) { acc[r][2 * j] = b0; acc[r][2 * j + 1] = b1; }
    }

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += KT) {
        __syncthreads();                  // the tile before this one has been read by everybody
        park();
        __syncthreads();
        if (k0 + KT < K) fetch(k0 + KT);  // in flight under the products below
#pragma unroll 2
        for (int k4 = 0; k4 < KT; k4 += 4) {
            float4 x[TR];
#pragma unroll
            for (int r = 0; r < TR; ++r) x[r] = *reinterpret_cast<const float4 *>(&xs[(ty + 32 * r) * XLD + k4]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                double wv[TC];
#pragma unroll
                for (int j = 0; j < TC / 2; ++j) {
                    const double2 p = *reinterpret_cast<const double2 *>(&ws[(k4 + kk) * NOUT + (j * 8 + tx) * 2]);
                    wv[2 * j] = p.x; wv[2 * j + 1] = p.y;
                }
#pragma unroll
                for (int r = 0; r < TR; ++r) {
                    const double xv = (double)(kk == 0 ? x[r].x : kk == 1 ? x[r].y : kk == 2 ? x[r].z : x[r].w);
#pragma unroll
                    for (int c = 0; c < TC; ++c) acc[r][c] = fma(xv, wv[c], acc[r][c]);
                }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int64_t row = row0 + ty + 32 * r;
        if (row >= n_rows) continue;
        float *dst = out + row * n_out;
#pragma unroll
        for (int j = 0; j < TC / 2; ++j) {
            const int o = (j * 8 + tx) * 2;
            if (o < n_out) dst[o] = (float)acc[r][2 * j];
            if (o + 1 < n_out) dst[o + 1] = (float)acc[r][2 * j + 1];
        }
    }
}

template <int NOUT, bool VEC>
void launch(unsigned grid, hipStream_t s, const float *abd, int n_abd, const float *tnf, int n_tnf, int64_t n_rows, const double *w, const double *b,
            int n_out, float *out)
{
    hipLaunchKernelGGL((affine_rows_kernel<NOUT, VEC>), dim3(grid), dim3(THREADS), 0, s, abd, n_abd, tnf, n_tnf, n_rows, w, b, n_out, out);
}

}  // namespace

extern "C" int pg_affine_rows(const float *abd, int n_abd, const float *tnf, int n_tnf, int64_t n_rows, const double *w, const double *b, int n_out,
                              float *out, void *stream)
{
    if (n_abd < 0) return pg_fail(PG_EINVAL, "pg_affine_rows: n_abd = %d is negative", n_abd);
    if (n_tnf < 0) return pg_fail(PG_EINVAL, "pg_affine_rows: n_tnf = %d is negative", n_tnf);
    const int64_t K = (int64_t)n_abd + n_tnf;
    if (K < 1 || K > (1LL << 30)) return pg_fail(PG_EINVAL, "pg_affine_rows: n_abd + n_tnf = %lld, not in [1, 2^30]", (long long)K);
    if (n_out < 1 || n_out > PG_AFFINE_MAX_OUT) return pg_fail(PG_EINVAL, "pg_affine_rows: n_out = %d, not in [1, %d]", n_out, PG_AFFINE_MAX_OUT);
    if (n_rows < 0) return pg_fail(PG_EINVAL, "pg_affine_rows: n_rows = %lld is negative", (long long)n_rows);
    if (n_rows == 0) return PG_OK;
    if (n_abd > 0 && !abd) return pg_fail(PG_EINVAL, "pg_affine_rows: abd is null");
    if (n_tnf > 0 && !tnf) return pg_fail(PG_EINVAL, "pg_affine_rows: tnf is null");
    if (!w) return pg_fail(PG_EINVAL, "pg_affine_rows: w is null");
    if (!b) return pg_fail(PG_EINVAL, "pg_affine_rows: b is null");
    if (!out) return pg_fail(PG_EINVAL, "pg_affine_rows: out is null");
    const int64_t grid = (n_rows + ROWS - 1) / ROWS;
    if (grid > 0x7fffffffLL) return pg_fail(PG_EINVAL, "pg_affine_rows: n_rows = %lld, too many rows for one launch", (long long)n_rows);
    const bool vec = n_abd % 4 == 0 && n_tnf % 4 == 0 && (uintptr_t)abd % 16 == 0 && (uintptr_t)tnf % 16 == 0;
    const hipStream_t s = (hipStream_t)stream;
    const unsigned g = (unsigned)grid;
    if (n_out <= 32) {
        if (vec) launch<32, true>(g, s, abd, n_abd, tnf, n_tnf, n_rows, w, b, n_out, out);
        else launch<32, false>(g, s, abd, n_abd, tnf, n_tnf, n_rows, w, b, n_out, out);
    } else {
        if (vec) launch<64, true>(g, s, abd, n_abd, tnf, n_tnf, n_rows, w, b, n_out, out);
        else launch<64, false>(g, s, abd, n_abd, tnf, n_tnf, n_rows, w, b, n_out, out);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail(PG_EHIP, "pg_affine_rows: %s", hipGetErrorString(e));
    return PG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The fold itself, one layer per launch, from the back: in front of the map out = y . a + c stands the layer
// y = BatchNorm(Linear(h)), eval mode -- y[j] = (sum_i h[i] weight[j, i] + bias[j] - mean[j]) * s[j] + beta[j] with
// s[j] = gamma[j] / sqrt(var[j] + eps) -- so out = h . a_out + c_out with
//     a_out[i, o] = sum_j weight[j, i] * (s[j] * a[j, o])        c_out[o] = c[o] + sum_j ((bias[j] - mean[j]) * s[j] + beta[j]) * a[j, o]
// in float64 from the float32 parameters.  One launch instead of the fourteen small kernels the same step takes as tensor
// operations (six casts, the BatchNorm scalars, two matrix-vector and one matrix-matrix product) -- per encode that was
// more time than the rows themselves.  A workgroup owns FOLD_TI rows of a_out (the last one c_out); thread (part, o) sums
// every fourth or eighth j, and the parts are added in order: the result depends on nothing but the operands.
namespace {

constexpr int FOLD_TI = 4;

struct FoldLayer {
    const float *weight, *bias, *mean, *var, *gamma, *beta;          // bias, gamma, beta may be null; mean == null: no BatchNorm
    double eps;
    int n_in, n_mid;
};

__global__ __launch_bounds__(THREADS) void affine_fold_kernel(FoldLayer l, const double *__restrict__ a, const double *__restrict__ c, int n_out,
                                                              double *__restrict__ a_out, double *__restrict__ c_out)
{
    __shared__ double part_sum[FOLD_TI][THREADS];                       // [ii][part * lanes + o]
    __shared__ double s_of[THREADS], t_of[THREADS];                     // s[j] and (bias[j] - mean[j]) * s[j] + beta[j] of a chunk of j
    const int lanes = n_out <= 32 ? 32 : 64, parts = THREADS / lanes;   // thread (part, o) sums j = part, part + parts, ..
    const int o = threadIdx.x % lanes, part = threadIdx.x / lanes;
    const bool offset_block = blockIdx.x == gridDim.x - 1;              // c_out; the blocks before it: rows i0 .. of a_out
    const int i0 = blockIdx.x * FOLD_TI;
    double acc[FOLD_TI] = {};
    for (int j0 = 0; j0 < l.n_mid; j0 += THREADS) {
        __syncthreads();                                                // the chunk before this one has been used by everybody
        const int jt = j0 + threadIdx.x;
        if (jt < l.n_mid) {                                             // (the square root and the division once per j, not per thread)
            double s = 1.0, shift = 0.0;
            if (l.mean) {
                s = (l.gamma ? (double)l.gamma[jt] : 1.0) / sqrt((double)l.var[jt] + l.eps);
                shift = (l.beta ? (double)l.beta[jt] : 0.0) - (double)l.mean[jt] * s;
            }
            s_of[threadIdx.x] = s;
            t_of[threadIdx.x] = (l.bias ? (double)l.bias[jt] : 0.0) * s + shift;
        }
        __syncthreads();
        const int n = l.n_mid - j0 < THREADS ? l.n_mid - j0 : THREADS;
        if (o >= n_out) continue;
#pragma unroll 8
        for (int jj = part; jj < n; jj += parts) {
            const int j = j0 + jj;
            const double aj = a ? a[(int64_t)j * n_out + o] : (j == o ? 1.0 : 0.0);      // (no a: the identity)
            if (offset_block) {
                acc[0] = fma(t_of[jj], aj, acc[0]);
            } else {
                const double p = s_of[jj] * aj;
#pragma unroll
                for (int ii = 0; ii < FOLD_TI; ++ii)
                    if (i0 + ii < l.n_in) acc[ii] = fma((double)l.weight[(int64_t)j * l.n_in + i0 + ii], p, acc[ii]);
            }
        }
    }
#pragma unroll
    for (int ii = 0; ii < FOLD_TI; ++ii) part_sum[ii][threadIdx.x] = acc[ii];
    __syncthreads();
    if (part != 0 || o >= n_out) return;
#pragma unroll
    for (int ii = 0; ii < FOLD_TI; ++ii) {
        double sum = part_sum[ii][o];
        for (int q = 1; q < parts; ++q) sum += part_sum[ii][q * lanes + o];
        if (offset_block) {
            if (ii == 0) c_out[o] = (c ? c[o] : 0.0) + sum;
        } else if (i0 + ii < l.n_in) {
            a_out[(int64_t)(i0 + ii) * n_out + o] = sum;
        }
    }
}

}  // namespace

extern "C" int pg_affine_fold(const float *weight, const float *bias, const float *bn_mean, const float *bn_var, const float *bn_gamma,
                              const float *bn_beta, double bn_eps, int n_in, int n_mid, const double *a, const double *c, int n_out,
                              double *a_out, double *c_out, void *stream)
{
    if (n_in < 1 || n_in > (1 << 24)) return pg_fail(PG_EINVAL, "pg_affine_fold: n_in = %d, not in [1, 2^24]", n_in);
    if (n_mid < 1 || n_mid > (1 << 24)) return pg_fail(PG_EINVAL, "pg_affine_fold: n_mid = %d, not in [1, 2^24]", n_mid);
    if (n_out < 1 || n_out > PG_AFFINE_MAX_OUT) return pg_fail(PG_EINVAL, "pg_affine_fold: n_out = %d, not in [1, %d]", n_out, PG_AFFINE_MAX_OUT);
    if (!weight) return pg_fail(PG_EINVAL, "pg_affine_fold: weight is null");
    if (!bn_mean != !bn_var) return pg_fail(PG_EINVAL, "pg_affine_fold: bn_mean and bn_var go together");
    if (!bn_mean && (bn_gamma || bn_beta)) return pg_fail(PG_EINVAL, "pg_affine_fold: bn_gamma / bn_beta without bn_mean");
    if (!a && n_mid != n_out) return pg_fail(PG_EINVAL, "pg_affine_fold: a is null (the identity) but n_mid = %d != n_out = %d", n_mid, n_out);
    if (!a_out) return pg_fail(PG_EINVAL, "pg_affine_fold: a_out is null");
    if (!c_out) return pg_fail(PG_EINVAL, "pg_affine_fold: c_out is null");
    const FoldLayer l = {weight, bias, bn_mean, bn_var, bn_gamma, bn_beta, bn_eps, n_in, n_mid};
    const unsigned grid = (unsigned)((n_in + FOLD_TI - 1) / FOLD_TI) + 1;
    hipLaunchKernelGGL(affine_fold_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, l, a, c, n_out, a_out, c_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail(PG_EHIP, "pg_affine_fold: %s", hipGetErrorString(e));
    return PG_OK;
}
