// Additive noise of task=asr on raw audio: 16-bit PCM in HBM + up to 8 noise sources per row, each
// a recording of a resident bank read from a phase and wrapped, scaled to a host-drawn SNR:
//   v_j[m] = w_j[(s_j + m) mod L_j],   Ex = sum x[m]^2,   Ev_j = sum_{m<n} v_j[m]^2   (int64, exact),
//   g_j = float(sqrt(double(Ex) / double(Ev_j) * r_j)),   r_j = 10^(-snr_j / 10) from the host,
//   y[m] = sat16(rint(fmaf(g_k, v_k[m], ... fmaf(g_1, v_1[m], float(x[m]))))),   0 for m >= n.
// The energies are integers, so their sums do not depend on the order; the gain is formed with
// IEEE double division and square root; a sample's bits depend on x[m], the v_j[m] and the row's
// gains only.
//
// Two launches.  mix_energy_kernel: block (chunk, row, slot) sums the squares of MX_CHUNK samples
// of x (slot 0) or of v_j (slot 1 + j) and writes one int64 partial; the block of an absent or
// refused source writes 0 and leaves, so rows with 0, 1 and 8 sources share one grid without one
// block doing nine times another's work.  mix_apply_kernel: block (tile, row) requests thread t's
// samples [8 t, 8 t + 8) of the row, adds up the row's partials (one wave per slot, lanes over the
// chunks), forms the gains and adds the same samples of every source whose gain is not 0.  Eight
// samples move as one
// 16-byte access wherever all eight lie inside the row's n samples and before the recording's
// wrap (the 2-byte-aligned case is covered by the target's unaligned access mode); one sample at
// a time at the row's end and across a wrap.  Every thread reads x[m] before it writes y[m] and no
// other thread touches that m, so out may be pcm itself.
#include "common.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int MX_THREADS = 256, MX_VEC = 8, MX_TILE = MX_THREADS * MX_VEC;
constexpr int MX_CHUNK = 2 * MX_TILE;  // samples per energy partial
constexpr int MX_MAX_SRC = 8, MX_SLOTS = MX_MAX_SRC + 1;

struct MixSrc {
  int64_t off, len, start;
  double r;
};

struct MixVec {
  int16_t s[MX_VEC];
};

// Source j of a row, or false: j outside the row's count, a count above 8, a source range outside
// the table, a recording or phase outside the bank, or an r that is no finite non-negative number.
__device__ inline bool mix_source(const int64_t* __restrict__ sources, int64_t n_src, int64_t bank_len, int first,
                                  int count, int j, MixSrc& s) {
  s.off = s.len = s.start = 0;
  s.r = 0.0;
  if (count < 0 || count > MX_MAX_SRC || j >= count || first < 0 || (int64_t)first > n_src - count) return false;
  const int64_t* e = sources + 4 * ((int64_t)first + j);
  s.off = e[0], s.len = e[1], s.start = e[2], s.r = __longlong_as_double(e[3]);
  return s.len >= 1 && s.off >= 0 && s.off <= bank_len - s.len && s.start >= 0 && s.start < s.len && s.r >= 0.0 &&
         s.r < INFINITY;
}

// (start + m) mod len for 0 <= start < len, 0 <= m < 2^30
__device__ inline int64_t mix_phase(int64_t start, int m, int64_t len) {
  const uint64_t t = (uint64_t)start + (uint64_t)m;
  if (t < (uint64_t)len) return (int64_t)t;
  if (len > 0x7fffffff) return (int64_t)(t - (uint64_t)len);  // m < len: one wrap at the most
  return (int64_t)((uint32_t)t % (uint32_t)len);              // t < 2^31 + 2^30
}

// x[0 .. cnt) and zeros
__device__ inline MixVec mix_load(const int16_t* __restrict__ x, int cnt) {
  MixVec v;
  if (cnt >= MX_VEC) {
    memcpy(&v, x, sizeof(v));
  } else {
#pragma unroll
    for (int i = 0; i < MX_VEC; ++i) v.s[i] = i < cnt ? x[i] : (int16_t)0;
  }
  return v;
}

// w[(idx + i) mod len], i < cnt, and zeros; 0 <= idx < len
__device__ inline MixVec mix_load_wrapped(const int16_t* __restrict__ w, int64_t len, int64_t idx, int cnt) {
  MixVec v;
  if (cnt >= MX_VEC && idx + MX_VEC <= len) {
    memcpy(&v, w + idx, sizeof(v));
  } else {
#pragma unroll
    for (int i = 0; i < MX_VEC; ++i) {
      v.s[i] = i < cnt ? w[idx] : (int16_t)0;
      if (++idx >= len) idx = 0;
    }
  }
  return v;
}

__device__ inline long long mix_sumsq(const MixVec& v) {
  long long a = 0;
#pragma unroll
  for (int i = 0; i < MX_VEC; ++i) a += (long long)((int)v.s[i] * (int)v.s[i]);
  return a;
}

__device__ inline long long mix_wave_sum(long long a) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
  return a;  // lane 0 holds the sum
}

__device__ inline int mix_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(MX_THREADS) void mix_energy_kernel(
    const int16_t* __restrict__ pcm, int64_t in_stride, int S, const int16_t* __restrict__ bank, int64_t bank_len,
    const int32_t* __restrict__ plan, const int64_t* __restrict__ sources, int64_t n_src,
    long long* __restrict__ ws, int nchunks) {
  __shared__ long long s_part[MX_THREADS / 64];
  const int b = blockIdx.y, c = blockIdx.x, slot = blockIdx.z, tid = threadIdx.x;
  const int n = mix_clamp(plan[3 * b], 0, S);
  const int m0 = c * MX_CHUNK;  // < S: the grid is cdiv(S, MX_CHUNK)
  if (m0 >= n) return;          // block-uniform; the apply kernel reads the chunks below n only
  long long* part = ws + ((int64_t)b * nchunks + c) * MX_SLOTS + slot;
  MixSrc s;
  if (slot > 0 && !mix_source(sources, n_src, bank_len, plan[3 * b + 1], plan[3 * b + 2], slot - 1, s)) {
    if (tid == 0) *part = 0;  // block-uniform: an absent or refused source
    return;
  }
  const int m_end = min(m0 + MX_CHUNK, n);
  // the chunk is two tiles: both loads of a lane are issued before either is summed
  const int g0 = m0 + tid * MX_VEC, g1 = g0 + MX_TILE;
  const int c0 = mix_clamp(m_end - g0, 0, MX_VEC), c1 = mix_clamp(m_end - g1, 0, MX_VEC);
  MixVec v0, v1;
  if (slot == 0) {
    const int16_t* x = pcm + (int64_t)b * in_stride;
    v0 = mix_load(x + g0, c0);
    v1 = mix_load(x + g1, c1);
  } else {
    v0 = mix_load_wrapped(bank + s.off, s.len, mix_phase(s.start, g0, s.len), c0);
    v1 = mix_load_wrapped(bank + s.off, s.len, mix_phase(s.start, g1, s.len), c1);
  }
  const long long a = mix_wave_sum(mix_sumsq(v0) + mix_sumsq(v1));
  if ((tid & 63) == 0) s_part[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < MX_THREADS / 64; ++w) t += s_part[w];
    *part = t;
  }
}

__global__ __launch_bounds__(MX_THREADS) void mix_apply_kernel(
    const int16_t* pcm, int64_t in_stride, int S, const int16_t* __restrict__ bank, int64_t bank_len,
    const int32_t* __restrict__ plan, const int64_t* __restrict__ sources, int64_t n_src,
    const long long* __restrict__ ws, int nchunks, int16_t* out, int64_t out_stride, float* __restrict__ gains) {
  __shared__ MixSrc s_src[MX_MAX_SRC];
  __shared__ int s_ok[MX_MAX_SRC];
  __shared__ float s_gain[MX_MAX_SRC];
  __shared__ long long s_e[MX_SLOTS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * MX_TILE;  // < S: the grid is cdiv(S, MX_TILE)
  const int n = mix_clamp(plan[3 * b], 0, S);
  const int first = plan[3 * b + 1], count = plan[3 * b + 2];
  int16_t* y = out + (int64_t)b * out_stride;
  const int mg = m0 + tid * MX_VEC;
  const int room = min(MX_VEC, S - mg);  // samples of the row this thread writes; may be <= 0
  const bool first_tile = blockIdx.x == 0;
  if (m0 >= n && !(first_tile && gains != nullptr)) {  // block-uniform: padding only
    MixVec z;
#pragma unroll
    for (int i = 0; i < MX_VEC; ++i) z.s[i] = 0;
    if (room >= MX_VEC) {
      memcpy(y + mg, &z, sizeof(z));
    } else {
#pragma unroll
      for (int i = 0; i < MX_VEC; ++i)
        if (i < room) y[mg + i] = 0;
    }
    return;
  }
  if (tid < MX_MAX_SRC) {
    MixSrc s;
    s_ok[tid] = mix_source(sources, n_src, bank_len, first, count, tid, s);
    s_src[tid] = s;
  }
  // this lane's samples of the row are requested before the partial sums are
  const int live = room <= 0 ? 0 : mix_clamp(n - mg, 0, MX_VEC);  // samples; the rest of `room` is padding
  const int16_t* x = pcm + (int64_t)b * in_stride;
  const MixVec xv = mix_load(x + mg, live);
  const int used = (n + MX_CHUNK - 1) / MX_CHUNK;  // <= nchunks
  for (int slot = tid >> 6; slot < MX_SLOTS; slot += MX_THREADS / 64) {
    long long a = 0;
    for (int c = tid & 63; c < used; c += 64) a += ws[((int64_t)b * nchunks + c) * MX_SLOTS + slot];
    a = mix_wave_sum(a);
    if ((tid & 63) == 0) s_e[slot] = a;
  }
  __syncthreads();
  if (tid < MX_MAX_SRC) {
    float g = 0.f;
    if (s_ok[tid] && s_e[0] > 0 && s_e[1 + tid] > 0)
      g = (float)sqrt((double)s_e[0] / (double)s_e[1 + tid] * s_src[tid].r);
    s_gain[tid] = g;
    if (first_tile && gains != nullptr && count >= 0 && count <= MX_MAX_SRC && tid < count && first >= 0 &&
        (int64_t)first <= n_src - count)
      gains[(int64_t)first + tid] = g;
  }
  __syncthreads();
  if (room <= 0) return;
  MixVec v;
  {
    float acc[MX_VEC];
#pragma unroll
    for (int i = 0; i < MX_VEC; ++i) acc[i] = (float)xv.s[i];
    // one source after the other: few registers and many waves per CU hide the loads better here
    // than requesting all sources first did (measured: 14.0 against 15.9 us for this kernel)
#pragma unroll
    for (int j = 0; j < MX_MAX_SRC; ++j) {
      const float g = s_gain[j];
      if (g == 0.f || live == 0) continue;  // g is block-uniform; fmaf(0, v, acc) is acc
      const MixSrc s = s_src[j];
      const MixVec w = mix_load_wrapped(bank + s.off, s.len, mix_phase(s.start, mg, s.len), live);
#pragma unroll
      for (int i = 0; i < MX_VEC; ++i) acc[i] = fmaf(g, (float)w.s[i], acc[i]);
    }
    // nearest-even, then saturation; a NaN (no finite gain gives one) would come out as -32768
#pragma unroll
    for (int i = 0; i < MX_VEC; ++i)
      v.s[i] = i < live ? (int16_t)fminf(fmaxf(rintf(acc[i]), -32768.f), 32767.f) : (int16_t)0;
  }
  if (room >= MX_VEC) {
    memcpy(y + mg, &v, sizeof(v));
  } else {
#pragma unroll
    for (int i = 0; i < MX_VEC; ++i)
      if (i < room) y[mg + i] = v.s[i];
  }
}

int64_t mix_chunks(int64_t S) { return cdiv(S, MX_CHUNK); }

}  // namespace

extern "C" int64_t lasr_mix_ws_bytes(int B, int64_t S) {
  if (B <= 0 || S <= 0) return 0;
  return (int64_t)B * mix_chunks(S) * MX_SLOTS * (int64_t)sizeof(long long);
}

extern "C" int lasr_mix_i16(const int16_t* pcm, int64_t in_stride, int B, int64_t S, const int16_t* bank,
                            int64_t bank_len, const int32_t* plan, const int64_t* sources, int64_t n_src, int16_t* out,
                            int64_t out_stride, float* gains, void* ws, int64_t ws_bytes, void* stream) {
  LASR_CHECK_ARG(B >= 0 && S >= 0 && bank_len >= 0 && n_src >= 0 && ws_bytes >= 0, "lasr_mix_i16: negative size");
  // sample indices are int in the kernels: a tile's end, S + MX_TILE, must not wrap
  LASR_CHECK_ARG(S <= (1 << 29), "lasr_mix_i16: more than 2^29 samples per row");
  LASR_CHECK_ARG(bank_len <= ((int64_t)1 << 46) && n_src <= ((int64_t)1 << 40),
                 "lasr_mix_i16: bank or table too large");
  if (B == 0 || S == 0) return LASR_OK;
  LASR_CHECK_ARG(pcm && out && plan, "lasr_mix_i16: null pointer");
  LASR_CHECK_ARG((bank || bank_len == 0) && (sources || n_src == 0), "lasr_mix_i16: null bank or source table");
  LASR_CHECK_ARG(((uintptr_t)pcm & 1) == 0 && ((uintptr_t)out & 1) == 0 && ((uintptr_t)bank & 1) == 0 &&
                     ((uintptr_t)plan & 3) == 0 && ((uintptr_t)sources & 7) == 0 && ((uintptr_t)gains & 3) == 0 &&
                     ((uintptr_t)ws & 7) == 0,
                 "lasr_mix_i16: misaligned pointer");
  LASR_CHECK_ARG(B == 1 || (in_stride >= S && out_stride >= S), "lasr_mix_i16: row stride smaller than S");
  LASR_CHECK_ARG(B <= 65535, "lasr_mix_i16: B too large for one launch");
  const int64_t is = B > 1 ? in_stride : 0, os = B > 1 ? out_stride : 0;
  const uintptr_t a0 = (uintptr_t)pcm, a1 = a0 + 2 * (uintptr_t)((int64_t)(B - 1) * is + S);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 2 * (uintptr_t)((int64_t)(B - 1) * os + S);
  LASR_CHECK_ARG((a0 == o0 && is == os) || a1 <= o0 || o1 <= a0,
                 "lasr_mix_i16: out overlaps pcm (in place needs the same pointer and stride)");
  const uintptr_t k0 = (uintptr_t)bank, k1 = k0 + 2 * (uintptr_t)bank_len;
  LASR_CHECK_ARG(bank_len == 0 || k1 <= o0 || o1 <= k0, "lasr_mix_i16: out overlaps the bank");
  const int64_t need = lasr_mix_ws_bytes(B, S);
  LASR_CHECK_ARG(ws && ws_bytes >= need, "lasr_mix_i16: workspace smaller than lasr_mix_ws_bytes(B, S)");
  const uintptr_t w0 = (uintptr_t)ws, w1 = w0 + (uintptr_t)need;
  LASR_CHECK_ARG((w1 <= o0 || o1 <= w0) && (w1 <= a0 || a1 <= w0), "lasr_mix_i16: workspace overlaps the rows");
  const int nchunks = (int)mix_chunks(S);
  mix_energy_kernel<<<dim3((unsigned)nchunks, (unsigned)B, MX_SLOTS), MX_THREADS, 0, (hipStream_t)stream>>>(
      pcm, is, (int)S, bank, bank_len, plan, sources, n_src, (long long*)ws, nchunks);
  int rc = lasr_check_launch("mix_i16 energy");
  if (rc != LASR_OK) return rc;
  mix_apply_kernel<<<dim3((unsigned)cdiv(S, MX_TILE), (unsigned)B), MX_THREADS, 0, (hipStream_t)stream>>>(
      pcm, is, (int)S, bank, bank_len, plan, sources, n_src, (const long long*)ws, nchunks, out, os, gains);
  return lasr_check_launch("mix_i16");
}
