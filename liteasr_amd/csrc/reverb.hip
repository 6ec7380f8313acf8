// Room reverberation of task=asr on raw audio: every row of the int16 batch convolved with a room
// impulse response (RIR) of a resident int16 bank, Kaldi's wav-reverberate --shift-output=true
// --normalize-output=true with the input's duration kept.  A row of n samples x, an RIR h of L
// samples whose largest sample (the first of them) is h[p]:
//   c[m] = sum_{k<L} (h[k] 2^-15) x[m + p - k],  0 <= m < n,  x = 0 outside [0, n)          (fp32)
//   Ex = sum x^2 (int64, exact),  Ec = sum_{m<n} c[m]^2 (double over the fp32 c, fixed order)
//   g = float(sqrt(double(Ex) / Ec)), 0 when Ex = 0 or Ec = 0
//   y[m] = sat16(rint(g c[m])),  0 for n <= m < S.
//
// Uniformly partitioned overlap-save with one block size RV_P = 2048, whatever the batch holds, so
// that a sample's bits depend on x[0..n), h, p and m only.  A 4096-point real transform is a
// 2048-point complex one, z[i] = w[2i] + i w[2i+1]: five radix-4 Stockham stages and one radix-2
// stage, ping-pong between two 16 KB LDS buffers, then the even / odd split.  A real spectrum is
// kept as 2048 complex numbers: bins 1 .. 2047, and (X[0], X[2048]), both real, in bin 0.
//
// Three launches.
//  reverb_fwd_kernel, block (slot, row): slot c < Cmax transforms the zero-padded partition
//    h[cP, cP + P) 2^-15 of the row's RIR; slot Cmax + t the window x[jP + p - P, jP + p + P),
//    j = t - (Cmax - 1).  Partitions past the RIR's own and windows that no output block of the row
//    reads, or that lie wholly outside [0, n), are skipped.
//  reverb_acc_kernel, block (a, row): Y = sum_c X_{a-c} H_c with c ascending (windows wholly
//    outside [0, n) left out), the inverse transform, whose last P points are c[aP .. aP + P), and
//    the block's sums of c^2 over m < n (double: per lane in index order, the wave's tree, the
//    waves ascending) and of x^2 (int64).
//  reverb_apply_kernel, block (tile, row): one lane adds the row's partials, blocks ascending,
//    and forms g; every lane scales, rounds and saturates eight samples.  Rows without an RIR
//    (index -1) are copied, rows with an RIR the kernels refuse are zero, padding is zero.  It
//    reads the workspace and, for a copied row, pcm at the samples it writes: out may be pcm.
//
// The second launch reads, per block, up to 2 C spectra of 16 KB from L2 and runs one transform; by
// arithmetic that traffic is what bounds it (C = 8 at 16000 taps).
#include "common.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int RV_P = 2048, RV_THREADS = 256;
constexpr int RV_MAX_L = 65536, RV_MAX_C = RV_MAX_L / RV_P;
constexpr int RV_VEC = 8, RV_TILE = RV_THREADS * RV_VEC;
constexpr float RV_HSCALE = 1.0f / 32768.0f;

struct RvRow {
  int n, mode;  // mode 0: a zero row, 1: a copy, 2: reverberated
  int64_t off;
  int len, peak, parts, blocks;
};

struct RvVec {
  int16_t s[RV_VEC];
};

__device__ inline int rv_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Row b of the plan.  An RIR is refused (mode 0) when its index is outside the table, it leaves the
// bank, its length is outside 1..65536 (or above what the workspace was sized for), or its peak
// lies outside it.
__device__ inline RvRow rv_row(const int32_t* __restrict__ plan, const int64_t* __restrict__ rirs, int64_t n_rir,
                               int64_t bank_len, int b, int S, int cmax) {
  RvRow r;
  r.n = rv_clamp(plan[2 * b], 0, S);
  r.mode = 0, r.off = 0, r.len = 0, r.peak = 0, r.parts = 0;
  r.blocks = (r.n + RV_P - 1) / RV_P;
  const int idx = plan[2 * b + 1];
  if (idx == -1) {
    r.mode = 1;
    return r;
  }
  if (idx < 0 || (int64_t)idx >= n_rir) return r;
  const int64_t* e = rirs + 3 * (int64_t)idx;
  const int64_t off = e[0], len = e[1], peak = e[2];
  if (len < 1 || len > RV_MAX_L || off < 0 || off > bank_len - len || peak < 0 || peak >= len) return r;
  const int parts = (int)((len + RV_P - 1) / RV_P);
  if (parts > cmax) return r;
  r.mode = 2, r.off = off, r.len = (int)len, r.peak = (int)peak, r.parts = parts;
  return r;
}

// Window j of a row holds x[lo, lo + 2P), lo = jP + p - P; false when none of it lies in [0, n).
__device__ inline bool rv_window(int j, int peak, int n, int& lo) {
  lo = j * RV_P + peak - RV_P;  // |j| <= 2^18 + 32: no wrap
  return lo + 2 * RV_P > 0 && lo < n;
}

LASR_DEV float2 rv_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// One radix-4 Stockham stage of the P-point forward transform, sub-transform length NS: butterflies
// tid and tid + 256.  tw[m] = exp(-2 pi i m / 2P), m < 2P.
template <int NS>
LASR_DEV void rv_stage4(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw,
                        int tid) {
  constexpr int Q = RV_P / 4;
#pragma unroll
  for (int q = 0; q < Q / RV_THREADS; ++q) {
    const int j = tid + RV_THREADS * q;
    const int k = j & (NS - 1);
    float2 v0 = in[j], v1 = in[j + Q], v2 = in[j + 2 * Q], v3 = in[j + 3 * Q];
    if (NS > 1) {
      const int m = k * (RV_P / (2 * NS));  // W_{4 NS}^k as a power of W_{2P}
      v1 = rv_cmul(v1, tw[m]);
      v2 = rv_cmul(v2, tw[2 * m]);
      v3 = rv_cmul(v3, tw[3 * m]);
    }
    const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
    const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y), a3 = make_float2(v1.x - v3.x, v1.y - v3.y);
    const int j0 = (j - k) * 4 + k;
    out[j0] = make_float2(a0.x + a2.x, a0.y + a2.y);
    out[j0 + NS] = make_float2(a1.x + a3.y, a1.y - a3.x);  // a1 - i a3
    out[j0 + 2 * NS] = make_float2(a0.x - a2.x, a0.y - a2.y);
    out[j0 + 3 * NS] = make_float2(a1.x - a3.y, a1.y + a3.x);  // a1 + i a3
  }
}

// The five radix-4 stages: the input in `a`, the result of sub-transform length 1024 in `b`.  The
// caller runs the last, radix-2 stage: out[j] = b[j] + W b[j + P/2], out[j + P/2] = b[j] - W b[j + P/2],
// W = tw[2 j].  A barrier is needed before `a` is written and the call ends with one.
LASR_DEV void rv_stages(float2* a, float2* b, const float2* __restrict__ tw, int tid) {
  rv_stage4<1>(a, b, tw, tid);
  __syncthreads();
  rv_stage4<4>(b, a, tw, tid);
  __syncthreads();
  rv_stage4<16>(a, b, tw, tid);
  __syncthreads();
  rv_stage4<64>(b, a, tw, tid);
  __syncthreads();
  rv_stage4<256>(a, b, tw, tid);
  __syncthreads();
}

__global__ __launch_bounds__(RV_THREADS) void reverb_fwd_kernel(
    const int16_t* __restrict__ pcm, int64_t in_stride, int S, const int16_t* __restrict__ bank, int64_t bank_len,
    const int32_t* __restrict__ plan, const int64_t* __restrict__ rirs, int64_t n_rir,
    const float2* __restrict__ tw, float2* __restrict__ spec, int cmax, int slots) {
  __shared__ float2 sa[RV_P];
  __shared__ float2 sb[RV_P];
  const int b = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const RvRow r = rv_row(plan, rirs, n_rir, bank_len, b, S, cmax);
  if (r.mode != 2 || r.blocks == 0) return;  // block-uniform, as every return below
  float* fa = reinterpret_cast<float*>(sa);
  if (s < cmax) {
    if (s >= r.parts) return;
    const int16_t* h = bank + r.off;
    const int k0 = s * RV_P;
#pragma unroll
    for (int q = 0; q < RV_P / RV_THREADS; ++q) {
      const int i = tid + RV_THREADS * q;
      fa[i] = k0 + i < r.len ? RV_HSCALE * (float)h[k0 + i] : 0.f;
      fa[RV_P + i] = 0.f;
    }
  } else {
    const int j = s - cmax - (cmax - 1);
    int lo;
    if (j < -(r.parts - 1) || j >= r.blocks || !rv_window(j, r.peak, r.n, lo)) return;
    const int16_t* x = pcm + (int64_t)b * in_stride;
#pragma unroll
    for (int q = 0; q < 2 * RV_P / RV_THREADS; ++q) {
      const int i = tid + RV_THREADS * q;
      const int m = lo + i;
      fa[i] = m >= 0 && m < r.n ? (float)x[m] : 0.f;
    }
  }
  __syncthreads();
  rv_stages(sa, sb, tw, tid);
#pragma unroll
  for (int q = 0; q < RV_P / 2 / RV_THREADS; ++q) {
    const int j = tid + RV_THREADS * q;
    const float2 v0 = sb[j], v1 = rv_cmul(sb[j + RV_P / 2], tw[2 * j]);
    sa[j] = make_float2(v0.x + v1.x, v0.y + v1.y);
    sa[j + RV_P / 2] = make_float2(v0.x - v1.x, v0.y - v1.y);
  }
  __syncthreads();
  // Z = sa -> the real transform's X[k] = E[k] + W_{2P}^k O[k]
  float2* X = spec + ((int64_t)b * slots + s) * RV_P;
#pragma unroll
  for (int q = 0; q < RV_P / RV_THREADS; ++q) {
    const int k = tid + RV_THREADS * q;
    const float2 zk = sa[k], zn = sa[(RV_P - k) & (RV_P - 1)];
    float2 v;
    if (k == 0) {
      v = make_float2(zk.x + zk.y, zk.x - zk.y);  // X[0] and X[P], both real
    } else {
      const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
      const float2 o = rv_cmul(tw[k], make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x)));
      v = make_float2(e.x + o.x, e.y + o.y);
    }
    X[k] = v;
  }
}

__global__ __launch_bounds__(RV_THREADS) void reverb_acc_kernel(
    const int16_t* __restrict__ pcm, int64_t in_stride, int S, int64_t bank_len, const int32_t* __restrict__ plan,
    const int64_t* __restrict__ rirs, int64_t n_rir, const float2* __restrict__ tw,
    const float2* __restrict__ spec, int cmax, int slots, float* __restrict__ conv, double* __restrict__ ec_part,
    long long* __restrict__ ex_part, int nblk) {
  __shared__ float2 sa[RV_P];
  __shared__ float2 sb[RV_P];
  __shared__ double s_ec[RV_THREADS / 64];
  __shared__ long long s_ex[RV_THREADS / 64];
  const int b = blockIdx.y, a = blockIdx.x, tid = threadIdx.x;
  const RvRow r = rv_row(plan, rirs, n_rir, bank_len, b, S, cmax);
  if (r.mode != 2 || a >= r.blocks) return;  // block-uniform
  const float2* base = spec + (int64_t)b * slots * RV_P;
  float2 acc[RV_P / RV_THREADS];
#pragma unroll
  for (int q = 0; q < RV_P / RV_THREADS; ++q) acc[q] = make_float2(0.f, 0.f);
  for (int c = 0; c < r.parts; ++c) {
    int lo;
    if (!rv_window(a - c, r.peak, r.n, lo)) continue;
    const float2* H = base + (int64_t)c * RV_P;
    const float2* X = base + (int64_t)(cmax + (a - c) + (cmax - 1)) * RV_P;
#pragma unroll
    for (int q = 0; q < RV_P / RV_THREADS; ++q) {
      const int k = tid + RV_THREADS * q;
      const float2 xv = X[k], hv = H[k];
      float2 p = rv_cmul(xv, hv);
      if (k == 0) p = make_float2(xv.x * hv.x, xv.y * hv.y);  // bins 0 and P, both real
      acc[q].x += p.x;
      acc[q].y += p.y;
    }
  }
#pragma unroll
  for (int q = 0; q < RV_P / RV_THREADS; ++q) sa[tid + RV_THREADS * q] = acc[q];
  __syncthreads();
  // Y = sa -> conj(Z) / 2P, Z[k] = (Y[k] + conj Y[P-k]) + i (Y[k] - conj Y[P-k]) conj(W_{2P}^k): the
  // inverse transform is the conjugate of the forward one of conj(Z)
  constexpr float sc = 0.5f / (float)RV_P;
#pragma unroll
  for (int q = 0; q < RV_P / RV_THREADS; ++q) {
    const int k = tid + RV_THREADS * q;
    const float2 yk = sa[k], yn = sa[(RV_P - k) & (RV_P - 1)];
    float2 z;
    if (k == 0) {
      z = make_float2(yk.x + yk.y, yk.x - yk.y);
    } else {
      const float2 e = make_float2(yk.x + yn.x, yk.y - yn.y), d = make_float2(yk.x - yn.x, yk.y + yn.y);
      const float2 w = tw[k];
      const float2 o = rv_cmul(d, make_float2(w.x, -w.y));
      z = make_float2(e.x - o.y, e.y + o.x);
    }
    sb[k] = make_float2(sc * z.x, -sc * z.y);
  }
  __syncthreads();
  rv_stages(sb, sa, tw, tid);
  // the last stage's second half is the last P real points: c[aP + 2j], c[aP + 2j + 1]
  float* cv = conv + ((int64_t)b * nblk + a) * RV_P;
  const int16_t* x = pcm + (int64_t)b * in_stride;
  const int m0 = a * RV_P;
  double ec = 0.0;
  long long ex = 0;
#pragma unroll
  for (int q = 0; q < RV_P / 2 / RV_THREADS; ++q) {
    const int j = tid + RV_THREADS * q;
    const float2 v0 = sa[j], v1 = rv_cmul(sa[j + RV_P / 2], tw[2 * j]);
    const float c0 = v0.x - v1.x, c1 = -(v0.y - v1.y);
    reinterpret_cast<float2*>(cv)[j] = make_float2(c0, c1);
    const int m = m0 + 2 * j;
    if (m < r.n) {
      ec += (double)c0 * (double)c0;
      const int v = x[m];
      ex += (long long)(v * v);
    }
    if (m + 1 < r.n) {
      ec += (double)c1 * (double)c1;
      const int v = x[m + 1];
      ex += (long long)(v * v);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    ec += __shfl_down(ec, d, 64);
    ex += __shfl_down(ex, d, 64);
  }
  if ((tid & 63) == 0) s_ec[tid >> 6] = ec, s_ex[tid >> 6] = ex;
  __syncthreads();
  if (tid == 0) {
    double te = 0.0;
    long long tx = 0;
#pragma unroll
    for (int w = 0; w < RV_THREADS / 64; ++w) te += s_ec[w], tx += s_ex[w];
    ec_part[(int64_t)b * nblk + a] = te;
    ex_part[(int64_t)b * nblk + a] = tx;
  }
}

__global__ __launch_bounds__(RV_THREADS) void reverb_apply_kernel(
    const int16_t* pcm, int64_t in_stride, int S, int64_t bank_len, const int32_t* __restrict__ plan,
    const int64_t* __restrict__ rirs, int64_t n_rir, int cmax, const float* __restrict__ conv,
    const double* __restrict__ ec_part, const long long* __restrict__ ex_part, int nblk, int16_t* out,
    int64_t out_stride, float* __restrict__ gains) {
  __shared__ float s_g;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * RV_TILE;  // < S: the grid is cdiv(S, RV_TILE)
  const RvRow r = rv_row(plan, rirs, n_rir, bank_len, b, S, cmax);
  int16_t* y = out + (int64_t)b * out_stride;
  const int mg = m0 + tid * RV_VEC;
  const int room = min(RV_VEC, S - mg);  // samples of the row this thread writes; may be <= 0
  const int live = room <= 0 || r.mode == 0 ? 0 : rv_clamp(r.n - mg, 0, RV_VEC);
  RvVec v;
#pragma unroll
  for (int i = 0; i < RV_VEC; ++i) v.s[i] = 0;
  if (r.mode == 2 && (m0 < r.n || blockIdx.x == 0)) {  // block-uniform
    if (tid == 0) {
      double ec = 0.0;
      long long ex = 0;
      for (int a = 0; a < r.blocks; ++a) {
        ec += ec_part[(int64_t)b * nblk + a];
        ex += ex_part[(int64_t)b * nblk + a];
      }
      const float g = ex > 0 && ec > 0.0 ? (float)sqrt((double)ex / ec) : 0.f;
      s_g = g;
      if (blockIdx.x == 0 && gains != nullptr) gains[b] = g;
    }
    __syncthreads();
    const float g = s_g;
    if (live > 0) {
      const float* cv = conv + (int64_t)b * nblk * RV_P + mg;  // mg + 8 <= blocks P: inside the row's blocks
      float c[RV_VEC];
      memcpy(c, cv, sizeof(c));
      // nearest-even, then saturation; a NaN (no finite input gives one) would come out as -32768
#pragma unroll
      for (int i = 0; i < RV_VEC; ++i)
        v.s[i] = i < live ? (int16_t)fminf(fmaxf(rintf(g * c[i]), -32768.f), 32767.f) : (int16_t)0;
    }
  } else {
    if (blockIdx.x == 0 && tid == 0 && gains != nullptr) gains[b] = r.mode == 1 ? 1.f : 0.f;
    if (r.mode == 1 && live > 0) {
      const int16_t* x = pcm + (int64_t)b * in_stride + mg;
      if (live >= RV_VEC) {
        memcpy(&v, x, sizeof(v));
      } else {
#pragma unroll
        for (int i = 0; i < RV_VEC; ++i) v.s[i] = i < live ? x[i] : (int16_t)0;
      }
    }
  }
  if (room >= RV_VEC) {
    memcpy(y + mg, &v, sizeof(v));
  } else {
#pragma unroll
    for (int i = 0; i < RV_VEC; ++i)
      if (i < room) y[mg + i] = v.s[i];
  }
}

int64_t rv_align(int64_t v) { return (v + 15) & ~(int64_t)15; }

// The workspace of B rows of S samples for RIRs of up to `parts` partitions: per row the spectra
// (slot c < parts: H_c; slot parts + t: window t - (parts - 1)), then the fp32 convolution, then
// the two partial sums per output block.
struct RvLayout {
  int64_t nblk, slots, spec, conv, ec, ex, total;
};

RvLayout rv_layout(int64_t B, int64_t S, int64_t parts) {
  RvLayout l;
  l.nblk = cdiv(S, (int64_t)RV_P);
  l.slots = l.nblk + 2 * parts - 1;
  l.spec = 0;
  l.conv = l.spec + rv_align(B * l.slots * RV_P * (int64_t)sizeof(float2));
  l.ec = l.conv + rv_align(B * l.nblk * RV_P * (int64_t)sizeof(float));
  l.ex = l.ec + rv_align(B * l.nblk * (int64_t)sizeof(double));
  l.total = l.ex + rv_align(B * l.nblk * (int64_t)sizeof(long long));
  return l;
}

}  // namespace

extern "C" int64_t lasr_reverb_ws_bytes(int B, int64_t S, int64_t Lmax) {
  if (B <= 0 || S <= 0 || S > (1 << 29)) return 0;
  const int64_t L = Lmax < 1 ? 1 : (Lmax > RV_MAX_L ? RV_MAX_L : Lmax);
  return rv_layout(B, S, cdiv(L, (int64_t)RV_P)).total;
}

extern "C" int lasr_reverb_i16(const int16_t* pcm, int64_t in_stride, int B, int64_t S, const int16_t* bank,
                               int64_t bank_len, const int32_t* plan, const int64_t* rirs, int64_t n_rir,
                               const float* tab, int16_t* out, int64_t out_stride, float* gains, void* ws,
                               int64_t ws_bytes, void* stream) {
  LASR_CHECK_ARG(B >= 0 && S >= 0 && bank_len >= 0 && n_rir >= 0 && ws_bytes >= 0, "lasr_reverb_i16: negative size");
  // sample indices are int in the kernels: a tile's end, S + RV_TILE, and a window's, must not wrap
  LASR_CHECK_ARG(S <= (1 << 29), "lasr_reverb_i16: more than 2^29 samples per row");
  LASR_CHECK_ARG(bank_len <= ((int64_t)1 << 46) && n_rir <= ((int64_t)1 << 31) - 1,
                 "lasr_reverb_i16: bank or table too large");
  if (B == 0 || S == 0) return LASR_OK;
  LASR_CHECK_ARG(pcm && out && plan && tab, "lasr_reverb_i16: null pointer");
  LASR_CHECK_ARG((bank || bank_len == 0) && (rirs || n_rir == 0), "lasr_reverb_i16: null bank or RIR table");
  LASR_CHECK_ARG(((uintptr_t)pcm & 1) == 0 && ((uintptr_t)out & 1) == 0 && ((uintptr_t)bank & 1) == 0 &&
                     ((uintptr_t)plan & 3) == 0 && ((uintptr_t)rirs & 7) == 0 && ((uintptr_t)gains & 3) == 0 &&
                     ((uintptr_t)tab & 7) == 0 && ((uintptr_t)ws & 15) == 0,
                 "lasr_reverb_i16: misaligned pointer");
  LASR_CHECK_ARG(B == 1 || (in_stride >= S && out_stride >= S), "lasr_reverb_i16: row stride smaller than S");
  LASR_CHECK_ARG(B <= 65535, "lasr_reverb_i16: B too large for one launch");
  const int64_t is = B > 1 ? in_stride : 0, os = B > 1 ? out_stride : 0;
  const uintptr_t a0 = (uintptr_t)pcm, a1 = a0 + 2 * (uintptr_t)((int64_t)(B - 1) * is + S);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 2 * (uintptr_t)((int64_t)(B - 1) * os + S);
  LASR_CHECK_ARG((a0 == o0 && is == os) || a1 <= o0 || o1 <= a0,
                 "lasr_reverb_i16: out overlaps pcm (in place needs the same pointer and stride)");
  const uintptr_t k0 = (uintptr_t)bank, k1 = k0 + 2 * (uintptr_t)bank_len;
  LASR_CHECK_ARG(bank_len == 0 || k1 <= o0 || o1 <= k0, "lasr_reverb_i16: out overlaps the bank");
  // the workspace's size says for how many partitions per RIR it was made
  const RvLayout one = rv_layout(B, S, 1), two = rv_layout(B, S, 2);
  LASR_CHECK_ARG(ws && ws_bytes >= one.total, "lasr_reverb_i16: workspace smaller than lasr_reverb_ws_bytes(B, S, 1)");
  int64_t parts = 1 + (ws_bytes - one.total) / (two.total - one.total);
  parts = parts > RV_MAX_C ? RV_MAX_C : parts;
  const RvLayout l = rv_layout(B, S, parts);
  const uintptr_t w0 = (uintptr_t)ws, w1 = w0 + (uintptr_t)l.total;
  LASR_CHECK_ARG((w1 <= o0 || o1 <= w0) && (w1 <= a0 || a1 <= w0) && (bank_len == 0 || w1 <= k0 || k1 <= w0),
                 "lasr_reverb_i16: workspace overlaps the rows or the bank");
  char* w = (char*)ws;
  const float2* tw = (const float2*)tab;
  float2* spec = (float2*)(w + l.spec);
  float* conv = (float*)(w + l.conv);
  double* ec = (double*)(w + l.ec);
  long long* ex = (long long*)(w + l.ex);
  reverb_fwd_kernel<<<dim3((unsigned)l.slots, (unsigned)B), RV_THREADS, 0, (hipStream_t)stream>>>(
      pcm, is, (int)S, bank, bank_len, plan, rirs, n_rir, tw, spec, (int)parts, (int)l.slots);
  int rc = lasr_check_launch("reverb_i16 forward");
  if (rc != LASR_OK) return rc;
  reverb_acc_kernel<<<dim3((unsigned)l.nblk, (unsigned)B), RV_THREADS, 0, (hipStream_t)stream>>>(
      pcm, is, (int)S, bank_len, plan, rirs, n_rir, tw, spec, (int)parts, (int)l.slots, conv, ec, ex, (int)l.nblk);
  rc = lasr_check_launch("reverb_i16 accumulate");
  if (rc != LASR_OK) return rc;
  reverb_apply_kernel<<<dim3((unsigned)cdiv(S, (int64_t)RV_TILE), (unsigned)B), RV_THREADS, 0, (hipStream_t)stream>>>(
      pcm, is, (int)S, bank_len, plan, rirs, n_rir, (int)parts, conv, ec, ex, (int)l.nblk, out, os, gains);
  return lasr_check_launch("reverb_i16");
}
