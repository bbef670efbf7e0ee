// Sampling decode step (new capability: the reference decodes greedily only,
// eval_utils/decode.py:53-81): temperature, top-k and nucleus (top-p) filtering and one
// Gumbel-max draw per logits row, one block per row.  Contract: include/retr_hip.h
// (retr_sample_rows) and DESIGN.md "Sampling decode".
//
// No sort and no prefix sum: the words are ranked by (z desc, index asc), z = logit / T, so a
// kept set is a cut (t, J) of that order: key > t, or key == t and index <= J, where key is the
// order-preserving 32-bit image of z.  Each of the two thresholds is found by 32 rounds of
// bisection on the key -- a round is one block reduction, an integer count for top-k and a
// probability mass for top-p -- and the words tied at a threshold are admitted by ascending
// index (a bisection on the index, run only when the ties are not all admitted).  The draw is
// argmax(z + Gumbel noise) over the kept words with the noise a pure function of
// (seed, step, row, word): retr_hash, the counter hash of the dropout masks.
//
// Every reduction has a fixed order (per-thread partial in a fixed traversal order, wave
// butterfly, the per-wave LDS array summed in wave order) and there are no atomics, so two
// launches on the same inputs give the same bits.  All control flow around the wave
// reductions is block-uniform (it depends on reduced values and kernel arguments only), so the
// 64 lanes of every wave are active in every one of them (common.hpp wave helpers).
//
// Temperature, top-k, top-p and the seed are read from device memory: a captured hipGraph
// freezes host scalars, and one captured decode step has to serve every setting.
#include "common.hpp"
#include "../../include/retr_hip.h"

namespace {

constexpr int kT = 512, kW = kT / 64, kC = 8;   // 512 threads x 8 chunks x 8 words in registers
constexpr int kRegWords = kT * kC * 8;          // 32768
constexpr int kNoCut = 0x7fffffff;

// lexicographic "better": larger value, then smaller index (first-index argmax semantics)
RETR_DEVICE bool better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

template <typename T>
RETR_DEVICE void load8f(const T* p, float (&v)[8]);
template <> RETR_DEVICE void load8f<bf16>(const bf16* p, float (&v)[8]) {
  const bf16x8 x = *(const bf16x8*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
}
template <> RETR_DEVICE void load8f<float>(const float* p, float (&v)[8]) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
  v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
  v[4] = b[0], v[5] = b[1], v[6] = b[2], v[7] = b[3];
}

// z = logit * (1 / temperature): one fp32 multiply (never fused into a later add); -0 -> +0 so
// that the key order below is the float order (first index among equal values)
RETR_DEVICE float scaled(float x, float inv_t) { return __fmul_rn(x, inv_t) + 0.0f; }
// order-preserving key of a float (a < b  <=>  key(a) < key(b)); 0 is kept free for "no word"
RETR_DEVICE unsigned key_of(float z) {
  const unsigned b = __float_as_uint(z);
  const unsigned k = b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
  return k ? k : 1u;
}
RETR_DEVICE float z_of(unsigned k) {
  return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu));
}

// chunk c (8 words) of a row whose first V words are valid: -inf beyond them
template <typename T>
RETR_DEVICE void load_chunk(const T* xr, int V, int c, float (&v)[8]) {
  if (c < V / 8) {
    load8f<T>(xr + 8 * (long)c, v);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long i = 8 * (long)c + e;
      v[e] = i < V ? to_f(xr[i]) : -INFINITY;
    }
  }
}

// f(logit, index) over this thread's words of the row, read from memory, in a fixed order
template <typename T, class F>
RETR_DEVICE void stream_row(const T* xr, int V, int tid, F f) {
  const int V8 = V / 8;
  for (int c = tid; c < V8; c += kT) {
    float v[8];
    load8f<T>(xr + 8 * (long)c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) f(v[e], 8 * c + e);
  }
  for (int j = 8 * V8 + tid; j < V; j += kT) f(to_f(xr[j]), j);
}

RETR_DEVICE int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += xor_lane(v, o);
  return v;
}

// Block reductions through red[2][kW]: consecutive reductions alternate the half they use, so
// one barrier each is enough (a wave writes half h again only after the barrier of the
// reduction in between, which every wave reaches after its reads of h).
struct BlockRed {
  unsigned (*red)[kW];
  int par, lane, wave;
  RETR_DEVICE unsigned* put(unsigned bits) {
    unsigned* r = red[par];
    if (lane == 0) r[wave] = bits;
    __syncthreads();
    par ^= 1;
    return r;
  }
  RETR_DEVICE float sum(float v) {
    const unsigned* r = put(__float_as_uint(wave_sum(v)));
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kW; ++w) s += __uint_as_float(r[w]);
    return s;
  }
  RETR_DEVICE float vmax(float v) {
    const unsigned* r = put(__float_as_uint(wave_max(v)));
    float s = -INFINITY;
#pragma unroll
    for (int w = 0; w < kW; ++w) s = fmaxf(s, __uint_as_float(r[w]));
    return s;
  }
  RETR_DEVICE int isum(int v) {
    const unsigned* r = put((unsigned)wave_isum(v));
    int s = 0;
#pragma unroll
    for (int w = 0; w < kW; ++w) s += (int)r[w];
    return s;
  }
};

// REG: the row's keys and softmax numerators live in registers (V <= 32768); otherwise every
// pass re-reads the row and recomputes them (same values, same traversal order per thread).
template <typename T, bool REG>
__global__ void __launch_bounds__(kT)
sample_kernel(const T* x, long ld, int V, const float* fparams, const long long* iparams,
              int step, const unsigned char* finished, long long* pred, float* logprob,
              int* n_kept) {
  __shared__ unsigned red[2][kW];
  __shared__ float wsc[kW];
  __shared__ int wix[kW];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* xr = x + (long)row * ld;
  const float inv_t = fparams[0], top_p = fparams[1];
  const long long top_k = iparams[0];
  const unsigned long long seed = (unsigned long long)iparams[1];
  BlockRed br{red, 0, tid & 63, tid >> 6};

  // pass 1: the row maximum (raw logits) and, in registers, every word's key
  unsigned key[kC][8];
  float ev[kC][8];
  float xmax = -INFINITY;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < kC; ++u) {
      const int c = tid + u * kT;
      float v[8];
      load_chunk<T>(xr, V, c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xmax = fmaxf(xmax, v[e]);
        key[u][e] = 8 * c + e < V ? key_of(scaled(v[e], inv_t)) : 0u;
      }
    }
  } else {
    stream_row<T>(xr, V, tid, [&](float xv, int) { xmax = fmaxf(xmax, xv); });
  }
  xmax = br.vmax(xmax);
  const float xs = xmax == -INFINITY ? 0.f : xmax;
  const float zmax = scaled(xmax, inv_t);
  const float zs = zmax == -INFINITY ? 0.f : zmax;

  // pass 2: log-sum-exp of the raw logits (the model's own log-likelihood) and the softmax
  // numerators exp(z - zmax) of the tempered ones
  float sraw = 0.f;
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < kC; ++u) {
      const int c = tid + u * kT;
      if (logprob) {
        float v[8];
        load_chunk<T>(xr, V, c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) sraw += expf(v[e] - xs);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        ev[u][e] = 8 * c + e < V ? expf(z_of(key[u][e]) - zs) : 0.f;
    }
  } else if (logprob) {
    stream_row<T>(xr, V, tid, [&](float xv, int) { sraw += expf(xv - xs); });
  }
  float lse = 0.f;
  if (logprob) lse = xs + logf(br.sum(sraw));

  // The top-k cut (tk, Jk): a word is in the top-k set iff key > tk, or key == tk and
  // index <= Jk ((1, none) = every word).  Once it is known, the words outside it read as
  // "no word" (key 0, numerator 0), so the nucleus passes need no membership test.
  unsigned tk = 1u;
  int Jk = kNoCut, nK = V;
  // f(key, numerator, index) over this thread's words
  auto each = [&](auto f) {
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < kC; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) f(key[u][e], ev[u][e], 8 * (tid + u * kT) + e);
    } else {
      stream_row<T>(xr, V, tid, [&](float xv, int j) {
        const float z = scaled(xv, inv_t);
        const unsigned k = key_of(z);
        const bool in = k > tk || (k == tk && j <= Jk);
        f(in ? k : 0u, in ? expf(z - zs) : 0.f, j);
      });
    }
  };
  auto count = [&](auto p) {
    int c = 0;
    each([&](unsigned k, float, int j) { c += p(k, j) ? 1 : 0; });
    return br.isum(c);
  };
  auto mass = [&](auto p) {
    float m = 0.f;
    each([&](unsigned k, float e, int j) { m += p(k, j) ? e : 0.f; });
    return br.sum(m);
  };
  // index of the need-th word (ascending index) among those with key t: the largest J with
  // fewer than `need` of them below J
  const int jbits = 32 - __clz(V > 1 ? V - 1 : 1);
  auto tie_cut = [&](unsigned t, int need) {
    int J = 0;
#pragma unroll 1
    for (int bit = jbits - 1; bit >= 0; --bit) {
      const int cand = J | (1 << bit);
      if (count([&](unsigned k, int j) { return k == t && j < cand; }) < need) J = cand;
    }
    return J;
  };

  // top-k: tk = the k-th largest key (the largest t with at least k keys >= t); of the words
  // tied at it, the first k - #{key > tk} by index.  Cut (tk, Jk), nK words.
  if (top_k > 0 && top_k < (long long)V) {
    const int k = (int)top_k;
    unsigned t = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = t | (1u << bit);
      if (count([&](unsigned kk, int) { return kk >= cand; }) >= k) t = cand;
    }
    tk = t ? t : 1u;
    const int c_gt = count([&](unsigned kk, int) { return kk > tk; });
    const int c_eq = count([&](unsigned kk, int) { return kk == tk; });
    const int need = k - c_gt;
    const int jk = need < c_eq ? tie_cut(tk, need) : kNoCut;
    Jk = jk;
    nK = k;
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < kC; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned kk = key[u][e];
          const bool in = kk > tk || (kk == tk && 8 * (tid + u * kT) + e <= Jk);
          key[u][e] = in ? kk : 0u;
          ev[u][e] = in ? ev[u][e] : 0.f;
        }
    }
  }

  // top-p over the top-k set: the largest t whose words (key >= t) hold at least
  // P = top_p * (the set's mass); the words tied at it all have the numerator e_t, so
  // ceil((P - mass above) / e_t) of them, by index, complete the prefix.  Cut (tp, Jp).
  unsigned tp = tk;
  int Jp = Jk, nkept = nK;
  if (top_p < 1.f) {
    const float P = top_p * mass([](unsigned, int) { return true; });
    unsigned t = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = t | (1u << bit);
      if (mass([&](unsigned k, int) { return k >= cand; }) >= P) t = cand;
    }
    tp = t > tk ? t : tk;
    const float m_gt = mass([&](unsigned k, int) { return k > tp; });
    const int n_gt = count([&](unsigned k, int) { return k > tp; });
    const int n_eq = count([&](unsigned k, int) { return k == tp; });
    const float mf = ceilf((P - m_gt) / expf(z_of(tp) - zs));
    const int m = mf >= 1.f ? (mf < (float)n_eq ? (int)mf : n_eq) : 1;
    nkept = n_gt + m;
    Jp = m < n_eq ? tie_cut(tp, m) : (tp == tk ? Jk : kNoCut);
  }

  // Gumbel-max draw over the kept words (the row is read again: no 64-fold unrolled hash)
  const unsigned long long draw = (unsigned long long)step * gridDim.x + (unsigned)row;
  const unsigned long long skey = seed ^ (draw * 0x9E3779B97F4A7C15ull);
  float bs = -INFINITY;
  int bi = kNoCut;
  stream_row<T>(xr, V, tid, [&](float xv, int j) {
    const float z = scaled(xv, inv_t);
    const unsigned k = key_of(z);
    if (k > tp || (k == tp && j <= Jp)) {
      const uint32_t h = retr_hash(skey, (uint64_t)j);
      const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;
      const float sc = __fadd_rn(z, -logf(-logf(u)));
      if (better(sc, j, bs, bi)) bs = sc, bi = j;
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s2 = xor_lane(bs, o);
    const int i2 = xor_lane(bi, o);
    if (better(s2, i2, bs, bi)) bs = s2, bi = i2;
  }
  if (br.lane == 0) wsc[br.wave] = bs, wix[br.wave] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kW; ++w)
      if (better(wsc[w], wix[w], bs, bi)) bs = wsc[w], bi = wix[w];
    if (bi < 0 || bi >= V) bi = 0;      // (a row of NaNs: no word compares better)
    pred[row] = bi;
    if (logprob) {
      const bool fin = finished && finished[row];
      logprob[row] = fin ? 0.f : to_f(xr[bi]) - lse;
    }
    if (n_kept) n_kept[row] = nkept;
  }
}

}  // namespace

extern "C" int retr_sample_rows(int dtype, const void* logits, long ld, int M, int V,
                                const float* fparams, const long long* iparams, int step,
                                const unsigned char* finished, long long* pred, float* logprob,
                                int* n_kept, void* stream) {
  RETR_REQUIRE(dtype == RETR_F32 || dtype == RETR_BF16, "sample_rows: dtype %d", dtype);
  RETR_REQUIRE(M >= 0 && V >= 1 && ld >= V && ld % 8 == 0,
               "sample_rows: M=%d V=%d ld=%ld (ld >= V >= 1, ld %% 8 == 0)", M, V, ld);
  RETR_REQUIRE(((uintptr_t)logits & 15) == 0, "sample_rows: logits must be 16-byte aligned");
  RETR_REQUIRE(fparams && iparams && pred, "sample_rows: fparams, iparams and pred are required");
  RETR_REQUIRE(step >= 0, "sample_rows: step=%d", step);
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool reg = V <= kRegWords;
#define SAMPLE(TT, RR)                                                                         \
  hipLaunchKernelGGL((sample_kernel<TT, RR>), dim3(M), dim3(kT), 0, st, (const TT*)logits, ld, \
                     V, fparams, iparams, step, finished, pred, logprob, n_kept)
  if (dtype == RETR_BF16) {
    if (reg) SAMPLE(bf16, true); else SAMPLE(bf16, false);
  } else {
    if (reg) SAMPLE(float, true); else SAMPLE(float, false);
  }
#undef SAMPLE
  return retr_check_launch("sample_rows");
}
