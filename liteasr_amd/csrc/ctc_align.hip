// CTC forced alignment: the Viterbi pass over the extended-label lattice and its backtrace.
//
// Input is what lasr_ctc_fwd's first stage (ctc_lse_gather_kernel, ctc.hip) leaves behind: lp
// [B][T][Lmax+1] fp32, column 0 the blank log-prob of the frame, column 1+i that of target i.
// One workgroup per utterance, one lattice state per thread (S_b = 2 L_b + 1 <= 1024), as
// ctc_alpha: the same skip rule, decided once, and the same emission prefetch ring, here
// ALIGN_W steps deep.
//
//   v_0(0) = lp[0][blank], v_0(1) = lp[0][y_1], every other state -inf
//   v_t(s) = best + lp[t][e(s)]:  best = v_{t-1}(s), move 0; replaced by v_{t-1}(s-1), move 1,
//            only if strictly greater; then by v_{t-1}(s-2), move 2, only if strictly greater
//            and the skip is allowed (s odd, s >= 2, label(s) != label(s-2))
//
// One fp32 add per step after a max of fp32 values: nothing to reassociate or contract, so the
// scores are the bits of a float32 restatement (tests/ctc_align_ref.py).
//
// Moves take 2 bits.  A thread packs the moves of ALIGN_W = 16 consecutive frames of its own
// state into one dword (no cross-lane traffic) and writes it once per 16 steps: frame t >= 1 is
// bits 2 ((t - 1) % 16) of word [(t - 1) / 16][s].  When 4 Smax (2 + ceil(T / 16)) bytes -- the
// ping-pong score vectors and every move word of the launch's T x Smax lattice -- fit 64 KB, the
// words live in LDS and the backtrace (one thread, T dependent steps) never waits on HBM.
// Otherwise they are spilled to the caller's workspace, [B][ceil(T / 16)][Smax] dwords, and the
// backtrace stages one 16-frame row of words at a time in LDS (the next row's loads in flight
// while it walks).
#include "common.h"

constexpr int ALIGN_W = 16;                // frames per move word = depth of the emission ring
constexpr int64_t ALIGN_LDS = 64 * 1024;  // what the kernels here allow themselves

__host__ __device__ static inline int64_t align_words(int T) { return (T + ALIGN_W - 1) / ALIGN_W; }
static int64_t align_lds_bytes(int T, int Lmax) { return 4 * (int64_t)(2 * Lmax + 1) * (2 + align_words(T)); }

LASR_DEV void align_step_sync() {  // LDS only: the emission ring's loads stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <bool SPILL>
__global__ __launch_bounds__(1024) void ctc_align_kernel(int T_, int Lmax, const int32_t* __restrict__ targets,
                                                         const int32_t* __restrict__ ilen,
                                                         const int32_t* __restrict__ tlen,
                                                         const float* __restrict__ lp, uint32_t* ws,
                                                         int32_t* states, int32_t* spans, float* score) {
  // [2][Smax] fp32 score vectors (the spill path's word staging after the recursion), then,
  // LDS path only, [ceil(T_/16)][Smax] move words
  extern __shared__ float sh[];
  const int b = blockIdx.x;
  // lengths past the launch's own are clamped: nothing outside the buffers is touched
  const int Tb = min(ilen[b], T_), Lb = min(max(tlen[b], 0), Lmax), S = 2 * Lb + 1, Smax = 2 * Lmax + 1;
  const int s = threadIdx.x, nt = blockDim.x;
  int32_t* st = states + (int64_t)b * T_;
  int32_t* sp = spans + (int64_t)b * 2 * Lmax;
  // what lies past the row's own lengths
  for (int t = max(Tb, 0) + s; t < T_; t += nt) st[t] = -1;
  for (int j = 2 * Lb + s; j < 2 * Lmax; j += nt) sp[j] = -1;
  if (Tb <= 0) {
    for (int j = s; j < 2 * Lb; j += nt) sp[j] = -1;
    if (s == 0) score[b] = (Lb == 0) ? 0.f : -INFINITY;
    return;
  }
  const int32_t* tg = targets + (int64_t)b * Lmax;
  const bool act = s < S;
  const bool skip = act && s >= 2 && (s & 1) && tg[s >> 1] != tg[(s >> 1) - 1];
  // every thread loads every step, unconditionally (a load under a branch costs the ring its
  // counted waits): idle threads read the blank column, steps past the end re-read frame Tb-1
  const int eix = (act && (s & 1)) ? 1 + (s >> 1) : 0;
  const int64_t ld = Lmax + 1;
  const float* lpb = lp + (int64_t)b * T_ * ld + eix;
  float* buf0 = sh;
  float* buf1 = sh + Smax;
  uint32_t* words = SPILL ? ws + (int64_t)b * align_words(T_) * Smax : (uint32_t*)(sh + 2 * Smax);

  float* prev = buf0;
  float* cur = buf1;
  if (act) prev[s] = s <= 1 ? lpb[0] : -INFINITY;
  float epf[ALIGN_W];  // epf[k]: the emission of frame t0 + k
#pragma unroll
  for (int k = 0; k < ALIGN_W; ++k) epf[k] = lpb[min(1 + k, Tb - 1) * ld];
  __syncthreads();
  uint32_t mw = 0;
  auto step = [&](float e, int k) {
    if (act) {
      float best = prev[s];
      uint32_t mv = 0;
      if (s >= 1) {
        const float a1 = prev[s - 1];
        if (a1 > best) { best = a1; mv = 1; }
      }
      if (skip) {
        const float a2 = prev[s - 2];
        if (a2 > best) { best = a2; mv = 2; }
      }
      cur[s] = best + e;
      mw |= mv << (2 * k);
    }
    align_step_sync();
    float* tmp = prev; prev = cur; cur = tmp;
  };
  // frames 1 .. Tb-1 in rows of 16: frame t is bit pair (t - 1) % 16 of word row (t - 1) / 16.
  // Whole rows run without a branch, so the ring's loads are waited for by count.
  int t0 = 1;
  for (; t0 + ALIGN_W <= Tb; t0 += ALIGN_W) {
    mw = 0;
#pragma unroll
    for (int k = 0; k < ALIGN_W; ++k) {
      const float e = epf[k];
      epf[k] = lpb[(int64_t)min(t0 + k + ALIGN_W, Tb - 1) * ld];
      step(e, k);
    }
    if (act) words[(int64_t)(t0 / ALIGN_W) * Smax + s] = mw;
  }
  if (t0 < Tb) {  // the last, partial row: its emissions are in the ring already
    mw = 0;
#pragma unroll
    for (int k = 0; k < ALIGN_W - 1; ++k)
      if (t0 + k < Tb) step(epf[k], k);  // uniform
    if (act) words[(int64_t)(t0 / ALIGN_W) * Smax + s] = mw;
  }
  __syncthreads();  // the last words (LDS, or the workspace: a workgroup-scope release / acquire)

  // end state and score; the verdict goes to the other threads through cur
  if (s == 0) {
    int end = 0;
    float v = prev[0];
    if (S >= 2) {
      const float a = prev[S - 1], c = prev[S - 2];
      end = a >= c ? S - 1 : S - 2;
      v = a >= c ? a : c;
    }
    score[b] = v;
    ((int*)cur)[0] = isfinite(v) ? end : -1;
  }
  __syncthreads();
  const int end = ((const int*)cur)[0];
  if (end < 0) {  // no finite path: nothing but -1s
    for (int t = s; t < Tb; t += nt) st[t] = -1;
    for (int j = s; j < 2 * Lb; j += nt) sp[j] = -1;
    return;
  }

  // backtrace, thread 0: frames Tb-1 .. 0, one row of move words (16 frames) at a time
  int q = end, qn = -1;  // the state at frame t and at frame t + 1
  auto walk = [&](const uint32_t* row, int k) {
    for (int t = min(Tb - 1, k * ALIGN_W + ALIGN_W); t >= (k ? k * ALIGN_W + 1 : 0); --t) {
      const int mv = t > 0 ? (int)((row[q] >> (2 * ((t - 1) & (ALIGN_W - 1)))) & 3u) : 0;
      st[t] = q;
      if (q & 1) {
        if (q != qn) sp[q] = t + 1;        // spans[q >> 1][1]: one past the label's last frame
        if (t == 0 || mv) sp[q - 1] = t;   // spans[q >> 1][0]: its first frame
      }
      qn = q;
      q -= mv;
    }
  };
  const int kb = max(Tb - 2, 0) / ALIGN_W;  // the row of the last frame's move
  if constexpr (!SPILL) {
    if (s == 0)
      for (int k = kb; k >= 0; --k) walk(words + (int64_t)k * Smax, k);
  } else {
    uint32_t* stage[2] = {(uint32_t*)buf0, (uint32_t*)buf1};
    __syncthreads();  // every thread has read the verdict out of cur
    if (act) stage[0][s] = words[(int64_t)kb * Smax + s];
    __syncthreads();
    for (int k = kb; k >= 0; --k) {
      const int c = (kb - k) & 1;
      uint32_t r = 0;
      if (k > 0 && act) r = words[(int64_t)(k - 1) * Smax + s];  // lands during the walk
      if (s == 0) walk(stage[c], k);
      if (k > 0 && act) stage[c ^ 1][s] = r;
      __syncthreads();
    }
  }
}

static int align_block(int S) {
  int nt = ((S + 63) / 64) * 64;
  return nt < 64 ? 64 : (nt > 1024 ? 1024 : nt);
}

extern "C" int64_t lasr_ctc_align_workspace(int B, int T, int Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0 || 2 * Lmax + 1 > 1024) return 0;
  if (align_lds_bytes(T, Lmax) <= ALIGN_LDS) return 0;
  return 4 * (int64_t)B * align_words(T) * (2 * Lmax + 1);
}

extern "C" int lasr_ctc_align(int B, int T, int Lmax, const int32_t* targets, const int32_t* ilen,
                              const int32_t* tlen, const float* lp, void* workspace, int64_t ws_bytes,
                              int32_t* states, int32_t* spans, float* score, void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && Lmax >= 0, "lasr_ctc_align: bad sizes");
  LASR_CHECK_ARG(2 * Lmax + 1 <= 1024, "lasr_ctc_align: Lmax=%d too large (one lattice state per thread)", Lmax);
  LASR_CHECK_ARG(ilen && tlen && lp && (targets || Lmax == 0), "lasr_ctc_align: targets / ilen / tlen / lp");
  LASR_CHECK_ARG(states && score && (spans || Lmax == 0), "lasr_ctc_align: states / spans / score");
  const int Smax = 2 * Lmax + 1;
  const int64_t need = lasr_ctc_align_workspace(B, T, Lmax);
  hipStream_t st = (hipStream_t)stream;
  if (need == 0) {
    ctc_align_kernel<false><<<B, align_block(Smax), align_lds_bytes(T, Lmax), st>>>(
        T, Lmax, targets, ilen, tlen, lp, nullptr, states, spans, score);
    return lasr_check_launch("ctc_align");
  }
  LASR_CHECK_ARG(workspace && ws_bytes >= need,
                 "lasr_ctc_align: workspace of %lld bytes, %lld needed (lasr_ctc_align_workspace)",
                 (long long)ws_bytes, (long long)need);
  ctc_align_kernel<true><<<B, align_block(Smax), 2 * Smax * sizeof(float), st>>>(
      T, Lmax, targets, ilen, tlen, lp, (uint32_t*)workspace, states, spans, score);
  return lasr_check_launch("ctc_align");
}
