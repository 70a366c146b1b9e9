// Order statistics of sample rows on the device (include/ascent.h: ascent_sample_quantiles): per (quantity q, group i, problem p)
// the valid samples in ascending order, the quantiles of numpy's "linear" definition read off that order, and the number of
// samples at or below each limit.  Nothing is accumulated in floating point: the values are compared as 64-bit keys whose
// unsigned order is the value order (negatives with every bit flipped, the others with the sign bit flipped; every NaN one key
// above all numbers; a sample that is not valid the largest key of all), so a result depends on the set of valid values only.
//
// The data has the problem index fastest.  Two mappings:
//   q_sort    a workgroup takes P consecutive problems of one group and sorts their rows in LDS, one quantity after the other:
//             P * Spad keys (Spad = samples rounded up to a power of two, P * Spad <= SORT_KEYS), loaded in runs of P doubles,
//             a bitonic network over all P rows at once; every probability and every limit then reads the sorted row.
//             The validity of the tile's samples is worked out once and kept in LDS beside the keys.
//   q_select  samples > SORT_KEYS: a workgroup per (q, i, p), the samples spread over its lanes, a bit per sample for the validity
//             in LDS, x_(lo) by radix select with 8-bit digits from the top (an LDS histogram of integer counts), x_(hi) by one
//             more pass (the count of keys <= x_(lo) and the smallest key above it), one pass per limit.
// The interpolation x_(lo) + g * (x_(hi) - x_(lo)) is one subtraction, one multiplication and one addition, never fused.
#include "ascent_quantile.hpp"
#include "ascent_host.hpp"
#include <cmath>

#pragma clang fp contract(off)

namespace ascent {
namespace {

constexpr int QT = 512;              // threads of a q_sort workgroup
constexpr int SORT_KEYS = 16384;     // keys of a q_sort tile: 128 KiB of the CU's 160 KiB LDS, plus a byte per key for the validity
constexpr size_t SORT_LDS_MAX = (size_t)(SORT_KEYS + 16) * sizeof(unsigned long long) + SORT_KEYS;      // P <= 16 rows of Spad + 1 keys, and the bytes
constexpr int ST = 256;              // threads of a q_select workgroup
constexpr int MASK_WORDS = ASCENT_DISPERSE_MAX_SAMPLES / 32;
constexpr unsigned GRID_Y = 65535;
constexpr unsigned long long KEY_INVALID = ~0ull, KEY_NAN = ~0ull - 1, SIGN = 0x8000000000000000ull;

struct Probs { double v[QUANTILE_MAX_PROBS]; };

__device__ __forceinline__ bool finite_bits(double x) { return ((((unsigned long long)__double_as_longlong(x)) >> 52) & 0x7FF) != 0x7FF; }
__device__ __forceinline__ unsigned long long key_of(double x) {
  if (x != x) return KEY_NAN;
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b & SIGN) ? ~b : (b | SIGN);
}
__device__ __forceinline__ double value_of(unsigned long long k) {
  if (k >= KEY_NAN) return NAN;
  return __longlong_as_double((long long)((k & SIGN) ? (k & ~SIGN) : ~k));
}

// h = pi (n - 1), lo = floor(h), g = h - lo, hi = min(lo + 1, n - 1); n >= 1
__device__ __forceinline__ void quantile_ranks(double pi, int n, int &lo, int &hi, double &g) {
  const double h = pi * (double)(n - 1), fl = floor(h);
  g = h - fl;
  lo = (int)fl;
  if (lo > n - 1) lo = n - 1;      // (pi <= 1 keeps h <= n - 1; this only guards the index)
  hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
}
__device__ __forceinline__ double interpolate(double xlo, double xhi, double g) {
#pragma clang fp contract(off)
  const double d = xhi - xlo;
  const double m = g * d;
  return xlo + m;
}

// grid (ceil(batch / P), groups of this launch); dynamic LDS: keys [P][Spad + 1] (the odd row keeps the P rows of a load on
// different banks), then valid [P][Spad] bytes.  P = 1 << lgP, Spad = 1 << lgS >= 2.
__global__ __launch_bounds__(QT) void q_sort(const double *__restrict__ values, int Q, int G, int V, int S, long batch, int lgP,
                                             int lgS, int i0, Probs probs, int n_probs, const double *__restrict__ limits,
                                             int n_limits, double *__restrict__ count, double *__restrict__ quant,
                                             double *__restrict__ below) {
  extern __shared__ unsigned long long q_lds[];
  const int P = 1 << lgP, Spad = 1 << lgS, row = Spad + 1;
  unsigned long long *keys = q_lds;
  unsigned char *valid = (unsigned char *)(keys + (size_t)P * row);
  const int t = threadIdx.x, i = i0 + (int)blockIdx.y;
  const long p0 = (long)blockIdx.x * P;
  const size_t B = (size_t)batch, NS = (size_t)S, NG = (size_t)G;
  for (int e = t; e < (P << lgS); e += QT) {
    const int pl = e & (P - 1), s = e >> lgP;
    const long p = p0 + pl;
    bool ok = s < S && p < batch;
    if (ok)
      for (int q = 0; q < V; q++) ok = ok && finite_bits(values[(((size_t)q * NG + i) * NS + s) * B + p]);
    valid[(pl << lgS) + s] = ok ? 1 : 0;
  }
  __syncthreads();
  for (int q = 0; q < Q; q++) {
    const double *v = values + ((size_t)q * NG + i) * NS * B;
    for (int e = t; e < (P << lgS); e += QT) {
      const int pl = e & (P - 1), s = e >> lgP;
      unsigned long long k = KEY_INVALID;
      if (valid[(pl << lgS) + s]) k = key_of(v[(size_t)s * B + (size_t)(p0 + pl)]);
      keys[pl * row + s] = k;
    }
    __syncthreads();
    const int lgH = lgS - 1, pairs = P << lgH;
    for (int k = 2; k <= Spad; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int e = t; e < pairs; e += QT) {
          const int pl = e >> lgH, pi = e & ((1 << lgH) - 1);
          const int a = ((pi & ~(j - 1)) << 1) | (pi & (j - 1)), b = a | j;
          const unsigned long long ka = keys[pl * row + a], kb = keys[pl * row + b];
          if ((ka > kb) == ((a & k) == 0)) {
            keys[pl * row + a] = kb;
            keys[pl * row + b] = ka;
          }
        }
        __syncthreads();
      }
    }
    // every probability and every limit of the P rows: the number of valid samples is where the invalid keys begin
    for (int e = t; e < P * (n_probs + n_limits + 1); e += QT) {
      const int pl = e & (P - 1), j = e >> lgP;
      const long p = p0 + pl;
      if (p >= batch) continue;
      const unsigned long long *kr = keys + pl * row;
      int n = 0;
      for (int len = S; len > 0;) {      // first index in [0, S) with an invalid key
        const int half = len >> 1;
        if (kr[n + half] != KEY_INVALID) { n += half + 1; len -= half + 1; } else len = half;
      }
      if (j < n_probs) {
        double r = NAN;
        if (n > 0) {
          int lo, hi;
          double g;
          quantile_ranks(probs.v[j], n, lo, hi, g);
          r = interpolate(value_of(kr[lo]), value_of(kr[hi]), g);
        }
        quant[(((size_t)j * Q + q) * NG + i) * B + p] = r;
      } else if (j < n_probs + n_limits) {
        const int l = j - n_probs;
        const double lim = limits[((size_t)l * Q + q) * B + p];
        int c = 0;
        for (int len = n; len > 0;) {      // first index in [0, n) whose value is not <= the limit (NaN: none is)
          const int half = len >> 1;
          if (value_of(kr[c + half]) <= lim) { c += half + 1; len -= half + 1; } else len = half;
        }
        below[(((size_t)l * Q + q) * NG + i) * B + p] = (double)c;
      } else if (q == 0 && count) {
        count[(size_t)i * B + p] = (double)n;
      }
    }
    __syncthreads();
  }
}

// grid (batch, rows (q, i) of this launch).  Every loop over the samples runs the same number of rounds in every lane.
__global__ __launch_bounds__(ST) void q_select(const double *__restrict__ values, int Q, int G, int V, int S, long batch, long r0,
                                               Probs probs, int n_probs, const double *__restrict__ limits, int n_limits,
                                               double *__restrict__ count, double *__restrict__ quant, double *__restrict__ below) {
  __shared__ unsigned mask[MASK_WORDS];
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_n, sh_cnt, sh_rank;
  __shared__ unsigned long long sh_min, sh_prefix;
  const int t = threadIdx.x;
  const long p = blockIdx.x, qi = r0 + blockIdx.y;
  const int q = (int)(qi / G), i = (int)(qi % G);
  const size_t B = (size_t)batch, NS = (size_t)S, NG = (size_t)G;
  const double *v = values + ((size_t)q * NG + i) * NS * B + (size_t)p;
  if (t == 0) sh_n = 0;
  __syncthreads();
  for (int s0 = 0; s0 < S; s0 += ST) {      // 64 consecutive samples per wavefront: two words of the mask
    const int s = s0 + t;
    bool ok = s < S;
    if (ok)
      for (int r = 0; r < V; r++) ok = ok && finite_bits(values[(((size_t)r * NG + i) * NS + s) * B + (size_t)p]);
    const unsigned long long bal = __ballot(ok);
    if ((t & 63) == 0) {
      const int w = (s0 + t) >> 5;      // s0 + t is a multiple of 64 here; w + 1 < MASK_WORDS as S <= 32 MASK_WORDS
      if (w < MASK_WORDS) mask[w] = (unsigned)bal;
      if (w + 1 < MASK_WORDS) mask[w + 1] = (unsigned)(bal >> 32);
      atomicAdd(&sh_n, (unsigned)__popcll(bal));
    }
  }
  __syncthreads();
  const int n = (int)sh_n;
  if (t == 0 && q == 0 && count) count[(size_t)i * B + (size_t)p] = (double)n;
  for (int j = 0; j < n_probs; j++) {
    if (n == 0) {
      if (t == 0) quant[(((size_t)j * Q + q) * NG + i) * B + (size_t)p] = NAN;
      continue;
    }
    int lo, hi;
    double g;
    quantile_ranks(probs.v[j], n, lo, hi, g);
    unsigned long long prefix = 0;
    unsigned rank = (unsigned)lo;
    for (int shift = 56; shift >= 0; shift -= 8) {
      hist[t] = 0;      // ST = 256 bins
      __syncthreads();
      for (int s0 = 0; s0 < S; s0 += ST) {
        const int s = s0 + t;
        if (s < S && ((mask[s >> 5] >> (s & 31)) & 1u)) {
          const unsigned long long k = key_of(v[(size_t)s * B]);
          if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      if (t == 0) {
        unsigned cum = 0;
        int d = 0;
        for (; d < 255; d++) {
          const unsigned c = hist[d];
          if (rank < cum + c) break;
          cum += c;
        }
        sh_prefix = prefix | ((unsigned long long)d << shift);
        sh_rank = rank - cum;
      }
      __syncthreads();
      prefix = sh_prefix;
      rank = sh_rank;
    }
    double xlo = value_of(prefix), xhi = xlo;
    if (hi != lo) {      // x_(lo) again if more than lo + 1 keys are <= it, else the smallest key above it
      if (t == 0) { sh_cnt = 0; sh_min = KEY_INVALID; }
      __syncthreads();
      unsigned c = 0;
      unsigned long long mn = KEY_INVALID;
      for (int s0 = 0; s0 < S; s0 += ST) {
        const int s = s0 + t;
        if (s < S && ((mask[s >> 5] >> (s & 31)) & 1u)) {
          const unsigned long long k = key_of(v[(size_t)s * B]);
          if (k <= prefix) c++;
          else if (k < mn) mn = k;
        }
      }
      if (c) atomicAdd(&sh_cnt, c);
      if (mn != KEY_INVALID) atomicMin(&sh_min, mn);
      __syncthreads();
      if (sh_cnt <= (unsigned)lo + 1u) xhi = value_of(sh_min);
      __syncthreads();
    }
    if (t == 0) quant[(((size_t)j * Q + q) * NG + i) * B + (size_t)p] = interpolate(xlo, xhi, g);
  }
  for (int l = 0; l < n_limits; l++) {
    const double lim = limits[((size_t)l * Q + q) * B + (size_t)p];
    if (t == 0) sh_cnt = 0;
    __syncthreads();
    unsigned c = 0;
    for (int s0 = 0; s0 < S; s0 += ST) {
      const int s = s0 + t;
      if (s < S && ((mask[s >> 5] >> (s & 31)) & 1u) && v[(size_t)s * B] <= lim) c++;
    }
    if (c) atomicAdd(&sh_cnt, c);
    __syncthreads();
    if (t == 0) below[(((size_t)l * Q + q) * NG + i) * B + (size_t)p] = (double)sh_cnt;
    __syncthreads();
  }
}

}  // namespace

int quantile_run(const QuantileIO &io, hipStream_t stream, char *err, size_t errlen) {
  static_assert(ST == 256 && ASCENT_DISPERSE_MAX_SAMPLES % 64 == 0, "q_select: a bin per thread, two mask words per wavefront round");
  Probs pr{};
  for (int j = 0; j < io.n_probs; j++) pr.v[j] = io.probs[j];
  const int n_limits = io.limits ? io.n_limits : 0;
  int lgS = 1;
  while ((1 << lgS) < io.samples) lgS++;
  if ((1 << lgS) <= SORT_KEYS) {
    int lgP = 0;
    while (lgP < 4 && (2 << (lgP + lgS)) <= SORT_KEYS && (1L << lgP) < io.batch) lgP++;
    const size_t P = (size_t)1 << lgP, Spad = (size_t)1 << lgS, lds = P * (Spad + 1) * sizeof(unsigned long long) + P * Spad;
    static bool lds_allowed[64] = {};      // per device, once: the largest tile (callers hold the device's lock)
    int dev = 0;
    ASC_CHK(err, errlen, hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !lds_allowed[dev]) {
      ASC_CHK(err, errlen, hipFuncSetAttribute((const void *)q_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SORT_LDS_MAX));
      if (dev >= 0 && dev < 64) lds_allowed[dev] = true;
    }
    for (int i0 = 0; i0 < io.G; i0 += (int)GRID_Y) {
      const unsigned gy = (unsigned)(io.G - i0) < GRID_Y ? (unsigned)(io.G - i0) : GRID_Y;
      hipLaunchKernelGGL(q_sort, dim3((unsigned)((io.batch + (long)P - 1) / (long)P), gy), dim3(QT), lds, stream, io.values, io.Q, io.G,
                         io.V, io.samples, io.batch, lgP, lgS, i0, pr, io.n_probs, io.limits, n_limits, io.count, io.quant, io.below);
      ASC_CHK(err, errlen, hipGetLastError());
    }
  } else {
    const long rows = (long)io.Q * io.G;
    for (long r0 = 0; r0 < rows; r0 += GRID_Y) {
      const unsigned gy = rows - r0 < (long)GRID_Y ? (unsigned)(rows - r0) : GRID_Y;
      hipLaunchKernelGGL(q_select, dim3((unsigned)io.batch, gy), dim3(ST), 0, stream, io.values, io.Q, io.G, io.V, io.samples, io.batch, r0,
                         pr, io.n_probs, io.limits, n_limits, io.count, io.quant, io.below);
      ASC_CHK(err, errlen, hipGetLastError());
    }
  }
  return ASCENT_OK;
}

}  // namespace ascent
