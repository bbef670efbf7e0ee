// CrossEntropyLoss with options (ignore_index, label smoothing, reduction mean / sum / none) over
// the vocabulary head.  Same shape as loss.hip -- one 256-thread block per logit row, or the
// register-resident one-pass training form -- with three additions:
//   * a row whose target equals ignore_index leaves before any reduction (its target is one
//     load of the same address by every thread, so the exit is uniform over the block), writes
//     loss 0 and a zero gradient row and never reads its logits;
//   * label smoothing eps: row = (1-eps)(lse - x[t]) + eps (lse - mean_j x[j]),
//     dlogits = g (softmax - (1-eps) onehot - eps/V): one extra per-thread sum of x;
//   * the mean's denominator N_valid is a device scalar written by count_kernel on the same
//     stream, so a captured hipGraph divides by the count of the targets it is replayed on.
// A target that is neither ignored nor in [0, V) reads nothing: the row loss is NaN and the
// gradient has no one-hot term.
#include "common.hpp"
#include "../../include/retr_hip.h"

namespace {

RETR_DEVICE void online_merge(float& m, float& s, float m2, float s2) {
  float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// N_valid = #{i : tgt[i] != ignore} as a float (single block; integer partials, so the order of
// the tree does not matter)
__global__ void __launch_bounds__(256)
count_kernel(const long long* tgt, int n, long long ignore, float* denom) {
  __shared__ int red[4];
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) c += tgt[i] != ignore ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += xor_lane(c, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) denom[0] = (float)(red[0] + red[1] + red[2] + red[3]);
}

// row loss from the row statistics (thread 0 of a row's block)
template <typename T>
RETR_DEVICE float row_loss(const T* xr, int V, long long t, float l, float sx, float eps) {
  const float xt = (t >= 0 && t < V) ? to_f(xr[t]) : __builtin_nanf("");
  const float nll = l - xt;
  if (eps == 0.f) return nll;
  return (1.f - eps) * nll + eps * (l - sx / (float)V);
}

template <typename T>
__global__ void __launch_bounds__(256)
ce_fwd_opt_kernel(const T* x, long ld, int V, const long long* tgt, long long ignore, float eps,
                  float* lse, float* loss_rows) {
  __shared__ float sm[4], ss[4], sq[4];
  const int row = blockIdx.x;
  const long long t = tgt[row];
  if (t == ignore) {                    // uniform over the block, before any reduction
    if (threadIdx.x == 0) lse[row] = 0.f, loss_rows[row] = 0.f;
    return;
  }
  const T* xr = x + (long)row * ld;
  float m = -INFINITY, s = 0.f, q = 0.f;
  for (int j = threadIdx.x; j < V; j += 256) {
    float v = to_f(xr[j]);
    q += v;
    if (v > m) {
      s = s * __expf(m - v) + 1.f;
      m = v;
    } else {
      s += __expf(v - m);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    float m2 = xor_lane(m, o), s2 = xor_lane(s, o);
    online_merge(m, s, m2, s2);
    q += xor_lane(q, o);
  }
  int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = m, ss[w] = s, sq[w] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int i = 1; i < 4; ++i) online_merge(M, S, sm[i], ss[i]);
    float l = M + logf(S);
    lse[row] = l;
    loss_rows[row] = row_loss(xr, V, t, l, (sq[0] + sq[1]) + (sq[2] + sq[3]), eps);
  }
}

// deterministic sum of the per-row losses (single block), divided by *denom when given
__global__ void __launch_bounds__(256)
reduce_rows_kernel(const float* v, int n, const float* denom, float* out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = denom ? red[0] / denom[0] : red[0];
}

// dlogits = g (softmax - (1-eps) onehot - eps/V), g = dloss[row * dstride] / *denom (denom NULL:
// no division); an ignored row is zeros; columns [V, lddx) are zeros.  RESCALE: the buffer
// already holds the gradient for dloss = 1 (ce_fused_opt_kernel), so every block returns at
// once when *dloss is 1.
template <typename T, typename TD, bool RESCALE>
__global__ void __launch_bounds__(256)
ce_bwd_opt_kernel(const T* x, long ld, int V, const long long* tgt, long long ignore, float eps,
                  const float* lse, const float* dloss, long dstride, const float* denom, TD* dx,
                  long lddx) {
  if (RESCALE && dloss[0] == 1.f) return;
  const int row = blockIdx.x;
  TD* dr = dx + (long)row * lddx;
  const long long t = tgt[row];
  if (t == ignore) {
    for (int j = threadIdx.x; j < lddx; j += 256) dr[j] = from_f<TD>(0.f);
    return;
  }
  const T* xr = x + (long)row * ld;
  const float l = lse[row];
  const float g = denom ? dloss[(long)row * dstride] / denom[0] : dloss[(long)row * dstride];
  const float hot = 1.f - eps, uni = eps / (float)V;
  for (int j = threadIdx.x; j < lddx; j += 256) {
    float d = 0.f;
    if (j < V) d = (__expf(to_f(xr[j]) - l) - (j == t ? hot : 0.f) - uni) * g;
    dr[j] = from_f<TD>(d);
  }
}

// ce_fused_kernel (loss.hip) with the options: the row's 16-byte chunks stay in registers, so
// the logits are read once for lse, sum x, the row loss and the gradient for dloss = 1,
// g = 1 / *denom (denom NULL: 1).  An ignored row writes its zero chunks without a load.
template <int NCH>
__global__ void __launch_bounds__(256)
ce_fused_opt_kernel(const bf16* x, long ld, int V, const long long* tgt, long long ignore,
                    float eps, float* lse, float* loss_rows, const float* denom, bf16* dx,
                    long lddx) {
  __shared__ float red[4], redq[4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long t = tgt[row];
  bf16* dr = dx + (long)row * lddx;
  const int ndch = (int)(lddx / 8);
  if (t == ignore) {                    // uniform over the block, before any reduction
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int j = tid + 256 * i;
      if (j < ndch) *(bf16x8*)(dr + 8 * j) = z;
    }
    if (tid == 0) lse[row] = 0.f, loss_rows[row] = 0.f;
    return;
  }
  const bf16* xr = x + (long)row * ld;
  const int nch = (V + 7) / 8;                  // chunks holding real columns
  bf16x8 c[NCH];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int j = tid + 256 * i;
    if (j < nch) c[i] = *(const bf16x8*)(xr + 8 * j);
  }
  const float dn = denom ? denom[0] : 1.f;      // in flight with the row's loads
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int j = tid + 256 * i;
    if (j < nch)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (8 * j + e < V) m = fmaxf(m, (float)c[i][e]);
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, xor_lane(m, o));
  if (lane == 0) red[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int j = tid + 256 * i;
    if (j < nch)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (8 * j + e < V) {
          const float v = (float)c[i][e];
          s += __expf(v - m);
          q += v;
        }
  }
  for (int o = 32; o > 0; o >>= 1) s += xor_lane(s, o), q += xor_lane(q, o);
  if (lane == 0) red[w] = s, redq[w] = q;
  __syncthreads();
  const float l = m + logf(red[0] + red[1] + red[2] + red[3]);
  if (tid == 0) {
    lse[row] = l;
    loss_rows[row] = row_loss(xr, V, t, l, (redq[0] + redq[1]) + (redq[2] + redq[3]), eps);
  }
  const float g = 1.f / dn;
  const float hot = 1.f - eps, uni = eps / (float)V;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int j = tid + 256 * i;
    if (j >= ndch) continue;
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = 8 * j + e;
      float d = 0.f;
      if (j < nch && col < V) d = (__expf((float)c[i][e] - l) - (col == t ? hot : 0.f) - uni) * g;
      o[e] = (bf16)d;
    }
    *(bf16x8*)(dr + 8 * j) = o;
  }
}

int launch_reduce(const float* loss_rows, int M, const float* denom, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(256), 0, st, loss_rows, M, denom, loss);
  return retr_check_launch("ce_reduce_opt");
}

}  // namespace

extern "C" {

int retr_ce_count(int M, const long long* targets, long long ignore_index, float* denom,
                  void* stream) {
  RETR_REQUIRE(M >= 0 && denom, "ce_count: denom is NULL");
  hipLaunchKernelGGL(count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, targets, M,
                     ignore_index, denom);
  return retr_check_launch("ce_count");
}

int retr_ce_fwd_opt(int dtype, const void* logits, long ld, int M, int V,
                    const long long* targets, long long ignore_index, float label_smoothing,
                    float* lse, float* loss_rows, float* loss, const float* denom,
                    void* stream) {
  RETR_REQUIRE(V > 0 && ld >= V, "ce_fwd_opt: ld %ld < V %d", ld, V);
  hipStream_t st = (hipStream_t)stream;
  if (M > 0) {
    if (dtype == RETR_BF16)
      hipLaunchKernelGGL(ce_fwd_opt_kernel<bf16>, dim3(M), dim3(256), 0, st, (const bf16*)logits,
                         ld, V, targets, ignore_index, label_smoothing, lse, loss_rows);
    else
      hipLaunchKernelGGL(ce_fwd_opt_kernel<float>, dim3(M), dim3(256), 0, st,
                         (const float*)logits, ld, V, targets, ignore_index, label_smoothing, lse,
                         loss_rows);
    if (retr_check_launch("ce_fwd_opt")) return 1;
  }
  return loss ? launch_reduce(loss_rows, M, denom, loss, st) : 0;
}

int retr_ce_bwd_opt(int dtype, const void* logits, long ld, int M, int V,
                    const long long* targets, long long ignore_index, float label_smoothing,
                    const float* lse, const float* dloss, long dloss_stride, const float* denom,
                    void* dlogits, long lddl, void* stream) {
  if (M == 0) return 0;
  RETR_REQUIRE(V > 0 && ld >= V && lddl >= V, "ce_bwd_opt: ld %ld / lddl %ld < V %d", ld, lddl,
               V);
  RETR_REQUIRE(dloss_stride == 0 || dloss_stride == 1, "ce_bwd_opt: dloss_stride is 0 or 1");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RETR_BF16)
    hipLaunchKernelGGL((ce_bwd_opt_kernel<bf16, bf16, false>), dim3(M), dim3(256), 0, st,
                       (const bf16*)logits, ld, V, targets, ignore_index, label_smoothing, lse,
                       dloss, dloss_stride, denom, (bf16*)dlogits, lddl);
  else
    hipLaunchKernelGGL((ce_bwd_opt_kernel<float, float, false>), dim3(M), dim3(256), 0, st,
                       (const float*)logits, ld, V, targets, ignore_index, label_smoothing, lse,
                       dloss, dloss_stride, denom, (float*)dlogits, lddl);
  return retr_check_launch("ce_bwd_opt");
}

int retr_ce_fwd_bwd_opt(int dtype, const void* logits, long ld, int M, int V,
                        const long long* targets, long long ignore_index, float label_smoothing,
                        float* lse, float* loss_rows, float* loss, const float* denom,
                        void* dlogits, long lddl, void* stream) {
  RETR_REQUIRE(dtype == RETR_BF16 && V > 0 && ld % 8 == 0 && lddl % 8 == 0 && lddl >= V &&
                   ld >= V && (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0,
               "ce_fwd_bwd_opt: bf16, 8-aligned rows");
  constexpr int kNch = 16;                       // 16 x 8 x 256 = 32768 columns per row
  RETR_REQUIRE(lddl <= 8L * 256 * kNch, "ce_fwd_bwd_opt: row of %ld columns too long", lddl);
  hipStream_t st = (hipStream_t)stream;
  if (M > 0) {
    hipLaunchKernelGGL(ce_fused_opt_kernel<kNch>, dim3(M), dim3(256), 0, st, (const bf16*)logits,
                       ld, V, targets, ignore_index, label_smoothing, lse, loss_rows, denom,
                       (bf16*)dlogits, lddl);
    if (retr_check_launch("ce_fwd_bwd_opt")) return 1;
  }
  return loss ? launch_reduce(loss_rows, M, denom, loss, st) : 0;
}

int retr_ce_bwd_rescale_opt(int dtype, const void* logits, long ld, int M, int V,
                            const long long* targets, long long ignore_index,
                            float label_smoothing, const float* lse, const float* dloss,
                            const float* denom, void* dlogits, long lddl, void* stream) {
  if (M == 0) return 0;
  RETR_REQUIRE(dtype == RETR_BF16 && V > 0 && ld >= V && lddl >= V,
               "ce_bwd_rescale_opt: bf16 only");
  hipLaunchKernelGGL((ce_bwd_opt_kernel<bf16, bf16, true>), dim3(M), dim3(256), 0,
                     (hipStream_t)stream, (const bf16*)logits, ld, V, targets, ignore_index,
                     label_smoothing, lse, dloss, 0L, denom, (bf16*)dlogits, lddl);
  return retr_check_launch("ce_bwd_rescale_opt");
}

}  // extern "C"
