// Speed perturbation of task=asr on raw audio: 16-bit PCM in HBM -> resampled 16-bit PCM, the
// Hann-windowed sinc of Kaldi's LinearResample (filter width L = 6, roll-off 0.99) in polyphase
// form, what `speed s` + `rate 16000` do offline.  A speed factor is a reduced fraction p / q; an
// utterance of N samples becomes ceil(q N / p), and output m = j q + i is
//   y[m] = sum_k x[j p - width + k] * tap[i][k],   k < 2 width + p,   x = 0 outside [0, N),
// rounded to nearest-even and saturated to int16 (the offline pipeline writes a 16-bit WAV here).
// The taps are computed in float64 on the host (liteasr_amd/kernels.py, resample_tables), one
// block of q x (2 width + p) per distinct ratio; rows of one batch carry different ratios.
//
// A block owns RS_TILE consecutive outputs of one row.  It stages the ratio's taps and the tile's
// input span, (tile / q) p + 2 width + p samples converted to fp32 and zero outside the row's own
// samples, in LDS.  Lane t then forms outputs m0 + t, m0 + t + 256, ...: consecutive lanes take
// consecutive outputs, so the q lanes of one j read the same span addresses (a broadcast) and
// the next j starts p floats on; the taps of the q phases lie 2 width + p floats apart.  One fp32
// accumulator per output, fmaf over k ascending: a sample's bits depend on its phase and its
// 2 width + p inputs only, not on the tile, the batch index, the strides or the alignment (samples
// are loaded and stored one int16 per lane).
#include "common.h"

namespace {

constexpr int RS_THREADS = 256, RS_TILE = 1024;
constexpr int RS_MAX_PQ = 32, RS_MAX_WIDTH = 13;  // width = ceil(6 / (0.99 * 0.5)) at speed 2
constexpr int RS_MAX_TAPS = RS_MAX_PQ * (2 * RS_MAX_WIDTH + RS_MAX_PQ);
// p <= 2 q: the tile's j range times p is at most 2 (RS_TILE - 1) + p, then 2 width + p more
constexpr int RS_MAX_SPAN = 2 * RS_TILE + 2 * RS_MAX_PQ + 2 * RS_MAX_WIDTH;

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const int16_t* __restrict__ pcm, int64_t in_stride, int S_in, const int32_t* __restrict__ plan,
    const int32_t* __restrict__ ratios, int n_ratios, const float* __restrict__ taps, int n_taps,
    int16_t* __restrict__ out, int64_t out_stride, int S_out) {
  __shared__ float s_tap[RS_MAX_TAPS];
  __shared__ float s_x[RS_MAX_SPAN];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * RS_TILE;  // < S_out: the grid is cdiv(S_out, RS_TILE)
  int16_t* y = out + (int64_t)b * out_stride;
  int n_in = plan[3 * b], n_out = plan[3 * b + 1];
  const int r = plan[3 * b + 2];
  n_in = n_in < 0 ? 0 : (n_in > S_in ? S_in : n_in);
  n_out = n_out < 0 ? 0 : (n_out > S_out ? S_out : n_out);
  int p = 0, q = 0, width = 0, off = 0;
  bool ok = r >= 0 && r < n_ratios;
  if (ok) {
    p = ratios[4 * r], q = ratios[4 * r + 1], width = ratios[4 * r + 2], off = ratios[4 * r + 3];
    ok = p >= 1 && q >= 1 && p <= RS_MAX_PQ && q <= RS_MAX_PQ && p <= 2 * q && width >= 0 &&
         width <= RS_MAX_WIDTH && off >= 0 && off <= n_taps && q * (2 * width + p) <= n_taps - off;
  }
  const int m_end = min(m0 + RS_TILE, S_out);         // this tile's outputs, [m0, m_end)
  const int live = ok ? min(m_end, n_out) : m0;       // of which [m0, live) are samples
  if (live <= m0) {  // block-uniform: padding only
    for (int m = m0 + tid; m < m_end; m += RS_THREADS) y[m] = 0;
    return;
  }
  const int nt = 2 * width + p;
  const int j0 = m0 / q, j1 = (live - 1) / q;
  const int span = (j1 - j0) * p + nt;   // <= RS_MAX_SPAN by the bounds on p, q and width above
  const int in0 = j0 * p - width;        // the row's sample at s_x[0]; below 0 in the first tile
  for (int k = tid; k < q * nt; k += RS_THREADS) s_tap[k] = taps[off + k];
  const int16_t* x = pcm + (int64_t)b * in_stride;
  for (int k = tid; k < span; k += RS_THREADS) {
    const int n = in0 + k;
    s_x[k] = (n >= 0 && n < n_in) ? (float)x[n] : 0.f;
  }
  __syncthreads();
  for (int m = m0 + tid; m < m_end; m += RS_THREADS) {
    int16_t v = 0;
    if (m < live) {
      const int j = m / q, i = m - j * q;
      const float* xs = s_x + (j - j0) * p;
      const float* tp = s_tap + i * nt;
      float acc = 0.f;
      for (int k = 0; k < nt; ++k) acc = fmaf(xs[k], tp[k], acc);
      // nearest-even, then saturation: |acc| stays far below 2^31, so the order does not matter
      v = (int16_t)fminf(fmaxf(rintf(acc), -32768.f), 32767.f);
    }
    y[m] = v;
  }
}

}  // namespace

extern "C" int lasr_resample_i16(const int16_t* pcm, int64_t in_stride, int B, int64_t S_in, const int32_t* plan,
                                 const int32_t* ratios, int n_ratios, const float* taps, int64_t n_taps,
                                 int16_t* out, int64_t out_stride, int64_t S_out, void* stream) {
  LASR_CHECK_ARG(B >= 0 && S_in >= 0 && S_out >= 0 && n_ratios >= 0 && n_taps >= 0, "lasr_resample_i16: negative size");
  // sample indices are int in the kernel: j p + 2 width + p <= 2 S_out + a tile's span must not wrap
  LASR_CHECK_ARG(S_in <= (1 << 29) && S_out <= (1 << 29) && n_taps <= (1 << 29),
                 "lasr_resample_i16: more than 2^29 samples per row or taps");
  if (B == 0 || S_out == 0) return LASR_OK;
  LASR_CHECK_ARG(out && plan && ratios && taps, "lasr_resample_i16: null pointer");
  LASR_CHECK_ARG(n_ratios >= 1, "lasr_resample_i16: empty ratio table");
  LASR_CHECK_ARG(((uintptr_t)out & 1) == 0 && ((uintptr_t)plan & 3) == 0 && ((uintptr_t)ratios & 3) == 0 &&
                     ((uintptr_t)taps & 3) == 0,
                 "lasr_resample_i16: misaligned pointer");
  LASR_CHECK_ARG(B == 1 || out_stride >= S_out, "lasr_resample_i16: output row stride smaller than S_out");
  if (S_in > 0) {
    LASR_CHECK_ARG(pcm && ((uintptr_t)pcm & 1) == 0, "lasr_resample_i16: null or misaligned pcm");
    LASR_CHECK_ARG(B == 1 || in_stride >= S_in, "lasr_resample_i16: input row stride smaller than S_in");
    const uintptr_t a0 = (uintptr_t)pcm, a1 = a0 + 2 * (uintptr_t)((int64_t)(B - 1) * (B > 1 ? in_stride : 0) + S_in);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 2 * (uintptr_t)((int64_t)(B - 1) * (B > 1 ? out_stride : 0) + S_out);
    LASR_CHECK_ARG(a1 <= o0 || o1 <= a0, "lasr_resample_i16: out overlaps pcm");
  }
  LASR_CHECK_ARG(B <= 65535, "lasr_resample_i16: B too large for one launch");
  resample_kernel<<<dim3((unsigned)cdiv(S_out, RS_TILE), (unsigned)B), RS_THREADS, 0, (hipStream_t)stream>>>(
      pcm, B > 1 ? in_stride : 0, (int)S_in, plan, ratios, n_ratios, taps, (int)n_taps, out,
      B > 1 ? out_stride : 0, (int)S_out);
  return lasr_check_launch("resample_i16");
}
