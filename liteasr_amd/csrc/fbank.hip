// Kaldi fbank front end of task=asr on raw audio: 16-bit PCM in HBM -> log-mel features
// (compute-fbank-feats with --snip-edges=true --dither=0 --remove-dc-offset=true
// --preemphasis-coefficient=0.97 --window-type=povey --use-power=true --use-energy=false
// --low-freq=20 --high-freq=0, 25 ms / 10 ms frames at 16 kHz, samples at int16 scale).
//
// One wave per frame, four frames of one utterance per block.  A lane loads 7 of the frame's 400
// samples (and each one's predecessor, for the pre-emphasis), the wave sums them for the DC
// offset, and the windowed frame goes to LDS as 256 complex points z[n] = w[2n] + i w[2n+1].
// The 512-point real FFT is a 256-point complex one: four radix-4 Stockham stages, one
// butterfly per lane and stage, ping-pong between two LDS buffers, then the even / odd split
// X[k] = E[k] + W512^k O[k] for k < 256 (Kaldi's mel banks never use the Nyquist bin).  Lane f
// (and f + 64) sums the power spectrum over the two runs of bins of mel filter f.  The
// arithmetic is fp32 over tables the host computed in float64 (liteasr_amd/kernels.py,
// fbank_tables); only the final logarithm is taken in double.  A frame's result depends only on its 400 samples: not on its place in the
// batch, the row stride or the alignment of pcm (samples are loaded one int16 per lane).
#include "common.h"

#include <float.h>

namespace {

constexpr int FB_LEN = 400, FB_SHIFT = 160, FB_HALF = 256;  // samples per frame / shift, FFT bins used
constexpr int FB_WAVES = 4;                                  // frames per block
constexpr float FB_PREEMPH = 0.97f;
constexpr float FB_LOG_EPS = -15.9423851528787420f;  // log(FLT_EPSILON): the floor, exact by construction
// table offsets (floats) in `tab`
constexpr int FB_TW256 = 512, FB_TW512 = 1024, FB_UP = 1536, FB_DOWN = 1792;

LASR_DEV float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// One radix-4 Stockham stage of the 256-point transform: butterfly j of sub-transform length NS.
template <int NS>
LASR_DEV void fb_stage(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw,
                       int j) {
  const int k = j & (NS - 1);
  float2 v0 = in[j], v1 = in[j + 64], v2 = in[j + 128], v3 = in[j + 192];
  if (NS > 1) {
    const int m = k * (64 / NS);
    v1 = cmul(v1, tw[m]);
    v2 = cmul(v2, tw[2 * m]);
    v3 = cmul(v3, tw[3 * m]);
  }
  const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y), a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
  const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y), a3 = make_float2(v1.x - v3.x, v1.y - v3.y);
  const int j0 = (j - k) * 4 + k;
  out[j0] = make_float2(a0.x + a2.x, a0.y + a2.y);
  out[j0 + NS] = make_float2(a1.x + a3.y, a1.y - a3.x);  // a1 - i a3
  out[j0 + 2 * NS] = make_float2(a0.x - a2.x, a0.y - a2.y);
  out[j0 + 3 * NS] = make_float2(a1.x - a3.y, a1.y + a3.x);  // a1 + i a3
}

__global__ __launch_bounds__(64 * FB_WAVES) void fbank_kernel(
    const int16_t* __restrict__ pcm, int64_t row_stride, const int32_t* __restrict__ nframes, int max_frames,
    const float* __restrict__ tab, const int32_t* __restrict__ seg, int F, const float* __restrict__ mean,
    const float* __restrict__ istd, float* __restrict__ out, int Tmax) {
  __shared__ float2 sa[FB_WAVES][FB_HALF];
  __shared__ float2 sb[FB_WAVES][FB_HALF];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int t = blockIdx.x * FB_WAVES + w;
  int nf = nframes[b];
  nf = nf < 0 ? 0 : (nf > max_frames ? max_frames : nf);  // the host checked S against max_frames
  const bool live = t < nf;  // wave-uniform; every wave walks through every barrier
  float2* za = sa[w];
  float2* zb = sb[w];
  float* fa = reinterpret_cast<float*>(za);

  // samples, DC offset, pre-emphasis (from the samples as loaded: w[i] -= 0.97 w[i-1] taken
  // from the back is x[i] - 0.97 x[i-1]; i = 0 uses itself), window; zero-padded to 512
  {
    const int16_t* x = pcm + (int64_t)b * row_stride + (int64_t)FB_SHIFT * t;
    float cur[7], prev[7];
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const int i = lane + 64 * q;
      const bool in = live && i < FB_LEN;
      cur[q] = in ? (float)x[i] : 0.f;
      prev[q] = in ? (float)x[i > 0 ? i - 1 : 0] : 0.f;
      s += cur[q];
    }
    const float mu = wave_sum(s) / (float)FB_LEN;  // integers below 2^24: exact in any order
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const int i = lane + 64 * q;
      const float v = ((cur[q] - mu) - FB_PREEMPH * (prev[q] - mu)) * tab[i];
      fa[i] = i < FB_LEN ? v : 0.f;
    }
    fa[lane + 448] = 0.f;
  }
  const float2* tw256 = reinterpret_cast<const float2*>(tab + FB_TW256);
  const float2* tw512 = reinterpret_cast<const float2*>(tab + FB_TW512);
  __syncthreads();
  fb_stage<1>(za, zb, tw256, lane);
  __syncthreads();
  fb_stage<4>(zb, za, tw256, lane);
  __syncthreads();
  fb_stage<16>(za, zb, tw256, lane);
  __syncthreads();
  fb_stage<64>(zb, za, tw256, lane);
  __syncthreads();
  // Z = za -> power spectrum of the 512-point real transform, into zb's storage
  float* pw = reinterpret_cast<float*>(zb);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = lane + 64 * q;
    const float2 zk = za[k], zn = za[(FB_HALF - k) & (FB_HALF - 1)];
    const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 o = cmul(tw512[k], make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x)));
    const float xr = e.x + o.x, xi = e.y + o.y;
    pw[k] = xr * xr + xi * xi;
  }
  __syncthreads();
  if (t >= Tmax) return;  // no barrier below
  float* y = out + ((int64_t)b * Tmax + t) * F;
  for (int f = lane; f < F; f += 64) {
    float r = 0.f;  // rows past the utterance's frames are zero, with CMVN too
    if (live) {
      const int s0 = min(max(seg[f], 0), FB_HALF), s1 = min(max(seg[f + 1], s0), FB_HALF);
      const int s2 = min(max(seg[f + 2], s1), FB_HALF);
      float e = 0.f;
      for (int k = s0; k < s1; ++k) e += tab[FB_UP + k] * pw[k];
      for (int k = s1; k < s2; ++k) e += tab[FB_DOWN + k] * pw[k];
      // The logarithm alone runs in double and rounds once: the output's own rounding is most of
      // the error budget (one ulp of a log value of 32 is 3.8e-6 of the energy), and logf, good to
      // an ulp or two, spent it (measured: 4.2e-6 against the 1.0e-6 of a correctly rounded log).
      r = e > FLT_EPSILON ? (float)log((double)e) : FB_LOG_EPS;
      if (mean) r = (r - mean[f]) * istd[f];
    }
    y[f] = r;
  }
}

}  // namespace

extern "C" int lasr_fbank(const int16_t* pcm, int64_t row_stride, int B, int64_t S, const int32_t* nframes,
                          int max_frames, const float* tab, const int32_t* seg, int F, const float* mean,
                          const float* istd, float* out, int Tmax, void* stream) {
  LASR_CHECK_ARG(B >= 0 && S >= 0 && Tmax >= 0 && max_frames >= 0, "lasr_fbank: negative size");
  LASR_CHECK_ARG(F >= 1 && F <= 128, "lasr_fbank: F must be in 1..128");
  if (B == 0 || Tmax == 0) return LASR_OK;
  LASR_CHECK_ARG(out && nframes && tab && seg, "lasr_fbank: null pointer");
  LASR_CHECK_ARG((mean == nullptr) == (istd == nullptr), "lasr_fbank: mean and istd go together");
  LASR_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)nframes & 3) == 0 && ((uintptr_t)tab & 7) == 0 &&
                     ((uintptr_t)seg & 3) == 0 && ((uintptr_t)mean & 3) == 0 && ((uintptr_t)istd & 3) == 0,
                 "lasr_fbank: misaligned pointer");
  if (max_frames > 0) {
    LASR_CHECK_ARG(pcm && ((uintptr_t)pcm & 1) == 0, "lasr_fbank: null or misaligned pcm");
    LASR_CHECK_ARG(S >= (int64_t)FB_SHIFT * (max_frames - 1) + FB_LEN,
                   "lasr_fbank: S = %lld samples cannot hold %d frames", (long long)S, max_frames);
    LASR_CHECK_ARG(B == 1 || row_stride >= S, "lasr_fbank: row stride smaller than S");
  }
  LASR_CHECK_ARG(B <= 65535, "lasr_fbank: B too large for one launch");
  fbank_kernel<<<dim3((unsigned)cdiv(Tmax, FB_WAVES), (unsigned)B), 64 * FB_WAVES, 0, (hipStream_t)stream>>>(
      pcm, row_stride, nframes, max_frames, tab, seg, F, mean, istd, out, Tmax);
  return lasr_check_launch("fbank");
}
