// cluster.hip -- pairwise-distance sums per cluster, the O(N^2) part of the silhouette score (pangaea_amd/clustering.py:
// dist_sums, silhouette_samples, choose_clusters):
//     out[i][c] = sum over the rows j of cluster c of |q_i - x_j|_2
// with x SORTED by cluster (seg[c] .. seg[c+1]-1 are the rows of cluster c).  A translation unit of its own, so that work on
// it cannot touch the timed kernels' code objects.
//
// The distance is formed from the differences -- subtract, square, accumulate over dim in float32, one square root -- never
// from |q|^2 + |x|^2 - 2 q.x, which loses the near pairs to cancellation.  The sum over j is float64: float32 partial sums of
// at most GROUP = 8 distances, each folded into the float64 sum of its (lane, cluster).
//
// One lane owns one query row: at dim 32 it keeps the row in 32 VGPRs for the whole kernel.  The reference row j is the same
// for every lane, so its address is wave-uniform and its values arrive by scalar loads into SGPRs; the inner loop is one
// subtract and one fused multiply-add per dimension with the SGPR as an operand.  The cluster boundary is uniform as well:
// "close the running sum, store it, start the next cluster" is a scalar branch, and the store is an ordinary vector store of
// one double per lane.  A workgroup of 256 lanes owns 256 query rows and ONE split of the reference range
// [n_x * s / n_splits, n_x * (s + 1) / n_splits); it walks all k clusters and writes a 0 for those outside its range, so
// every word of its [n_q, k] plane is written and nothing has to be cleared.  With one split the plane is `out`; with more,
// the planes lie in the workspace and a second kernel adds them in split order -- no floating-point atomics, the same bits
// from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pangaea_feat.h"
#include "pg_internal.h"

namespace {

constexpr int THREADS = 256;
constexpr int GROUP = PG_CLUSTER_GROUP;   // distances of one float32 partial sum
constexpr int TARGET_BLOCKS = 2048;       // 256 CUs x 8 workgroups of 256 lanes: what fills the device

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// DIM > 0: the query row lives in registers (dim == DIM).  DIM == 0: any dim; the lane reads its row once per GROUP of
// reference rows.
template <int DIM>
__global__ __launch_bounds__(THREADS) void dist_sums_kernel(const float *__restrict__ q, int64_t n_q, const float *__restrict__ x, int64_t n_x,
                                                            int dim, const int64_t *__restrict__ seg, int k, int n_splits,
                                                            double *__restrict__ dst)
{
    const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool live = row < n_q;
    const float *qrow = q + (live ? row : n_q - 1) * dim;          // (a lane beyond the rows computes the last row and stores nothing)
    const int64_t split = blockIdx.y;
    const int64_t j_lo = n_x * split / n_splits, j_hi = n_x * (split + 1) / n_splits;
    double *o = dst + (split * n_q + row) * k;

    float qr[DIM > 0 ? DIM : 1];
    if constexpr (DIM > 0) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) qr[d] = qrow[d];
    }

    // |q - x_j| for the uniform j
    auto dist = [&](int64_t j) -> float {
        const float *xr = x + j * (DIM > 0 ? DIM : dim);
        float d2 = 0.f;
        if constexpr (DIM > 0) {
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                const float t = qr[d] - xr[d];
                d2 = fmaf(t, t, d2);
            }
        }
        return sqrtf(d2);
    };

    for (int c = 0; c < k; ++c) {
        // the rows of cluster c inside this split; clamped, so that no content of seg can lead outside x
        const int64_t a = clamp64(seg[c], j_lo, j_hi), b = clamp64(seg[c + 1], j_lo, j_hi);
        double acc = 0.0;
        if constexpr (DIM > 0) {
            int64_t j = a;
            for (; j + GROUP <= b; j += GROUP) {
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < GROUP; ++t) s += dist(j + t);
                acc += (double)s;
            }
            if (j < b) {
                float s = 0.f;
                for (; j < b; ++j) s += dist(j);
                acc += (double)s;
            }
        } else {
            for (int64_t j = a; j < b; j += GROUP) {
                const int n = b - j < GROUP ? (int)(b - j) : GROUP;
                float d2[GROUP];
#pragma unroll
                for (int t = 0; t < GROUP; ++t) d2[t] = 0.f;
                for (int d = 0; d < dim; ++d) {
                    const float qv = qrow[d];
#pragma unroll
                    for (int t = 0; t < GROUP; ++t) {
                        const float v = qv - x[(j + (t < n ? t : n - 1)) * dim + d];    // (beyond the group: its last row again, not added)
                        d2[t] = fmaf(v, v, d2[t]);
                    }
                }
                float s = 0.f;
#pragma unroll
                for (int t = 0; t < GROUP; ++t)
                    if (t < n) s += sqrtf(d2[t]);
                acc += (double)s;
            }
        }
        if (live) o[c] = acc;
    }
}

// out[e] = plane 0 [e] + plane 1 [e] + .. in split order
__global__ __launch_bounds__(THREADS) void add_planes_kernel(const double *__restrict__ planes, int64_t n, int n_splits, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    double sum = planes[e];
    for (int s = 1; s < n_splits; ++s) sum += planes[(int64_t)s * n + e];
    out[e] = sum;
}

// the library's choice: one split when the query rows alone give enough workgroups, otherwise as many as fill the device, never
// more than PG_CLUSTER_MAX_SPLITS and never less than one GROUP-sized run of reference rows per split
int choose_splits(int64_t n_q, int64_t n_x)
{
    const int64_t q_blocks = (n_q + THREADS - 1) / THREADS;
    if (q_blocks < 1 || q_blocks * 2 > TARGET_BLOCKS) return 1;
    int64_t s = (TARGET_BLOCKS + q_blocks - 1) / q_blocks;
    const int64_t by_rows = n_x / (8 * GROUP);
    if (s > by_rows) s = by_rows;
    if (s > PG_CLUSTER_MAX_SPLITS) s = PG_CLUSTER_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

// PG_OK when the sizes are fine, else PG_EINVAL with the text for pg_last_error (shared by the two entries)
int check_sizes(const char *fn, int64_t n_q, int64_t n_x, int k, int n_splits)
{
    if (n_q < 0) return pg_fail(PG_EINVAL, "%s: n_q = %lld is negative", fn, (long long)n_q);
    if (n_x < 0) return pg_fail(PG_EINVAL, "%s: n_x = %lld is negative", fn, (long long)n_x);
    if (k < 1 || k > PG_CLUSTER_MAX_K) return pg_fail(PG_EINVAL, "%s: k = %d, not in [1, %d]", fn, k, PG_CLUSTER_MAX_K);
    if (n_splits < 0 || n_splits > PG_CLUSTER_MAX_SPLITS)
        return pg_fail(PG_EINVAL, "%s: n_splits = %d, not in [0, %d]", fn, n_splits, PG_CLUSTER_MAX_SPLITS);
    if (n_q > (1LL << 40) || n_x > (1LL << 40)) return pg_fail(PG_EINVAL, "%s: n_q = %lld / n_x = %lld beyond 2^40", fn, (long long)n_q, (long long)n_x);
    return PG_OK;
}

}  // namespace

extern "C" int64_t pg_cluster_dist_sums_workspace_bytes(int64_t n_q, int64_t n_x, int k, int n_splits)
{
    const int rc = check_sizes("pg_cluster_dist_sums_workspace_bytes", n_q, n_x, k, n_splits);
    if (rc != PG_OK) return rc;
    if (n_q == 0 || n_x == 0) return 0;
    const int s = n_splits > 0 ? n_splits : choose_splits(n_q, n_x);
    return s == 1 ? 0 : (int64_t)s * n_q * k * (int64_t)sizeof(double);
}

extern "C" int pg_cluster_dist_sums(const float *q, int64_t n_q, const float *x, int64_t n_x, int dim, const int64_t *seg, int k, int n_splits,
                                    double *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    static const char fn[] = "pg_cluster_dist_sums";
    const int rc = check_sizes(fn, n_q, n_x, k, n_splits);
    if (rc != PG_OK) return rc;
    if (dim < 1 || dim > PG_CLUSTER_MAX_DIM) return pg_fail(PG_EINVAL, "%s: dim = %d, not in [1, %d]", fn, dim, PG_CLUSTER_MAX_DIM);
    if (workspace_bytes < 0) return pg_fail(PG_EINVAL, "%s: workspace_bytes = %lld is negative", fn, (long long)workspace_bytes);
    if (n_q == 0 || n_x == 0) return PG_OK;
    if (!q) return pg_fail(PG_EINVAL, "%s: q is null", fn);
    if (!x) return pg_fail(PG_EINVAL, "%s: x is null", fn);
    if (!seg) return pg_fail(PG_EINVAL, "%s: seg is null", fn);
    if (!out) return pg_fail(PG_EINVAL, "%s: out is null", fn);
    const int splits = n_splits > 0 ? n_splits : choose_splits(n_q, n_x);
    const int64_t need = splits == 1 ? 0 : (int64_t)splits * n_q * k * (int64_t)sizeof(double);
    if (need > 0 && !workspace) return pg_fail(PG_EINVAL, "%s: workspace is null (%lld bytes needed for %d splits)", fn, (long long)need, splits);
    if (workspace_bytes < need)
        return pg_fail(PG_EINVAL, "%s: workspace_bytes = %lld, %lld needed for %d splits", fn, (long long)workspace_bytes, (long long)need, splits);
    const int64_t q_blocks = (n_q + THREADS - 1) / THREADS;
    const int64_t n_out = n_q * k, add_blocks = (n_out + THREADS - 1) / THREADS;
    if (q_blocks > 0x7fffffffLL || add_blocks > 0x7fffffffLL)
        return pg_fail(PG_EINVAL, "%s: n_q = %lld with k = %d, too many rows for one launch", fn, (long long)n_q, k);

    const hipStream_t s = (hipStream_t)stream;
    double *dst = splits == 1 ? out : (double *)workspace;
    const dim3 grid((unsigned)q_blocks, (unsigned)splits);
    if (dim == 32) hipLaunchKernelGGL(dist_sums_kernel<32>, grid, dim3(THREADS), 0, s, q, n_q, x, n_x, dim, seg, k, splits, dst);
    else hipLaunchKernelGGL(dist_sums_kernel<0>, grid, dim3(THREADS), 0, s, q, n_q, x, n_x, dim, seg, k, splits, dst);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && splits > 1) {
        hipLaunchKernelGGL(add_planes_kernel, dim3((unsigned)add_blocks), dim3(THREADS), 0, s, (const double *)workspace, n_out, splits, out);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return pg_fail(PG_EHIP, "%s: %s", fn, hipGetErrorString(e));
    return PG_OK;
}
