// Attention rescoring kept on the device (liteasr/models/u2.py:218-317), SURVEY §8 f3.
//
// Between the encoder and the answer of U2.inference nothing goes through the host:
//
//   search   CTC prefix beam search (u2.py:218-263) over the [Tcap, k] candidates that
//            lasr_logsoftmax_topk wrote; one workgroup, serial over the frames, T' read from a
//            device word.  Semantics of csrc/decode/prefix_beam.cpp step for step, in double.
//   prep     the decoder inputs of the n-best at the static shape (10, L1cap, Tcap): ys_in,
//            the decoder mask, the gather index and the memory mask (u2.py:268-298)
//   pick     float32 running sum of the gathered attention log-probs + float32(ctc score *
//            weight), first strict maximum (u2.py:300-315)
//
// Search, one frame.  The host loop runs candidate-major over (candidate j, hypothesis i) and
// each pair touches the entry of the hypothesis' own prefix (blank, repeat) and / or of its
// extension by the candidate.  The top-k ids of a frame are distinct and a prefix has one
// parent, so every field of every entry has a closed set of contributions:
//   pb  of a kept prefix x      one: the blank candidate                 {pb_x + p, pnb_x + p}
//   pnb of a kept prefix x      at most two, both under the candidate s = last(x): the repeat
//                               {pnb_x + p} and the extension of x's parent, when that is kept
//                               too ({pb + p, pnb + p}, or {pb + p} when the parent repeats s);
//                               the parent's position before / after x decides their order
//   pnb of a new extension      one
// Thread p = 10 j + i < 100 owns pair (j, i) and the entry of its extension when that is no
// kept prefix; threads 100..109 form pb and threads 110..119 pnb and the entry of kept prefix
// x.  Every log_add is the host's expression (left-to-right sum, the same exact shortcuts), so
// the fields are bit-equal up to the device's exp / log.  An entry's first touch in host loop
// order is the key 2 (10 j + i) + (second touch of a repeat pair); entries are ranked by
// (score descending, key ascending), which is Python's dict order under the stable sort, by
// counting the entries that come first.
//
// Prefix identity is exact and permanent: a prefix is a slot of an open-addressing table
// whose 64-bit key is (parent slot, token); the root is parent -1.  Slots are never freed
// within an utterance, so a prefix that is dropped and re-created is the same slot, and a
// descendant of its first incarnation still names it as parent.  Keys are compared in full;
// the hash only picks the first probe.  Lanes of a frame insert distinct keys, so a
// compare-and-swap on an empty slot is the whole insert.  Table traffic goes to L2 (agent-scope
// loads, atomics); everything else of a frame lives in LDS.
//
// Batch.  Every kernel takes B utterances: the batch arena is B single-utterance arenas laid end
// to end (stride = lasr_rescore_workspace(Tcap, Lcap) bytes), workgroup / grid row b works on
// arena b, on candidates [b Tcap k, ...), on Tp_dev[b], and on row b of the decoder inputs.  The
// utterances share nothing, so B workgroups of the serial search cost what one costs; a row with
// T' = 0 runs no frame, touches no table slot and reports n = 1, the empty prefix.  The
// single-utterance entries are the B = 1 launches.
//
// Built without contraction (Makefile: -ffp-contract=off for this file; the pragma below
// says the same) and without fast-math: + and the comparisons are the IEEE operations of the
// reference's Python floats.
#include "common.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int kBeam = 10;
constexpr int kThreads = 128;
constexpr int kPairs = kBeam * kBeam;
constexpr int kEnt = kBeam + kPairs;  // kept prefixes first, then one per pair
constexpr double kNinf = -__builtin_huge_val();
constexpr uint64_t kEmpty = ~0ull;

// result block (int32 words; include/liteasr_hip.h)
enum {
  R_ERR = 0,
  R_N = 1,
  R_BEST = 2,
  R_BESTLEN = 3,
  R_TP = 4,
  R_LENS = 8,
  R_SCORE = 20,  // 10 doubles
  R_TOTAL = 40,  // 10 floats
  R_HEAD = 64,
};
enum { E_OVERFLOW = 1, E_TABLE = 2, E_CAND = 4 };

struct Layout {
  int64_t best, toks, gath, head_words, table, table_cap, total;
};

__host__ __device__ inline Layout make_layout(int Tcap, int Lcap) {
  auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
  Layout L;
  L.best = R_HEAD;
  L.toks = L.best + Lcap;
  L.gath = L.toks + (int64_t)kBeam * Lcap;
  L.head_words = L.gath + (int64_t)kBeam * (Lcap + 1);
  int64_t hc = 1024;
  while (hc < 2 * ((int64_t)kPairs * Tcap + 1)) hc *= 2;
  L.table_cap = hc;
  L.table = up(L.head_words * 4);
  L.total = L.table + up(hc * 8);
  return L;
}

// u2.py:367-375 as csrc/decode/prefix_beam.cpp states it, for up to three arguments; a
// missing argument is -inf, which adds an exact 0.0 to the sum
LASR_DEV double la_term(double a, double m) { return a == kNinf ? 0.0 : (a == m ? 1.0 : exp(a - m)); }
LASR_DEV double log_add3(double a0, double a1, double a2) {
  if (a0 == kNinf && a1 == kNinf && a2 == kNinf) return kNinf;
  double m = a0;
  if (a1 > m) m = a1;
  if (a2 > m) m = a2;
  double s = 0.0;
  s += la_term(a0, m);
  s += la_term(a1, m);
  s += la_term(a2, m);
  return m + (s == 1.0 ? 0.0 : log(s));
}

LASR_DEV uint64_t ld_l2(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

LASR_DEV uint64_t node_key(int parent, int token) { return ((uint64_t)(uint32_t)parent << 32) | (uint32_t)token; }

// The slot of prefix (parent, token): found, or inserted.  -1 when the table is full (cannot
// happen at the documented capacity: at most 100 inserts per frame, load factor <= 1/2).
LASR_DEV int child_slot(uint64_t* table, int64_t cap, int parent, int token) {
  const uint64_t key = node_key(parent, token);
  const uint32_t mask = (uint32_t)cap - 1;
  uint32_t h = mix32((uint32_t)parent * 0x9E3779B1u ^ mix32((uint32_t)token)) & mask;
  for (int64_t probe = 0; probe < cap; ++probe, h = (h + 1) & mask) {
    uint64_t v = ld_l2(table + h);
    if (v == kEmpty) v = atomicCAS((unsigned long long*)(table + h), (unsigned long long)kEmpty, (unsigned long long)key);
    if (v == kEmpty || v == key) return (int)h;
  }
  return -1;
}

// every slot of the prefix tables empty: one 16-B store (two keys) per thread; grid row y = the
// utterance, its table `stride` bytes after the previous one
__global__ __launch_bounds__(256) void rescore_clear_kernel(char* __restrict__ table0, int64_t stride) {
  uint4* table = (uint4*)(table0 + (int64_t)blockIdx.y * stride);
  table[(int64_t)blockIdx.x * 256 + threadIdx.x] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

struct RankKey {
  double sc;
  int key;  // < 0: no entry
  int pad;
};

__global__ __launch_bounds__(kThreads) void rescore_search_kernel(int32_t* __restrict__ arena0, int Tcap, int Lcap, int k,
                                                                  int blank, const float* __restrict__ topv0,
                                                                  const int32_t* __restrict__ topi0,
                                                                  const int32_t* __restrict__ Tp_dev) {
  const Layout L = make_layout(Tcap, Lcap);
  const int b = blockIdx.x;  // the utterance: its arena, its candidates, its T'
  int32_t* arena = (int32_t*)((char*)arena0 + (int64_t)b * L.total);
  const float* topv = topv0 + (int64_t)b * Tcap * k;
  const int32_t* topi = topi0 + (int64_t)b * Tcap * k;
  uint64_t* table = (uint64_t*)((char*)arena + L.table);
  __shared__ int c_node[2][kBeam], c_last[2][kBeam], c_depth[2][kBeam];
  __shared__ double c_pb[2][kBeam], c_pnb[2][kBeam];
  __shared__ float cv[2][kBeam];
  __shared__ int ci[2][kBeam];
  __shared__ int ch[kPairs];          // extension slot of pair p, -2: none
  __shared__ double s_pb[kBeam];      // pb of kept prefix x this frame
  __shared__ int s_pbkey[kBeam];      // its first touch, -1: untouched
  __shared__ RankKey rk[kEnt];
  __shared__ int s_ncur, s_err;

  const int tid = threadIdx.x;
  int Tp = Tp_dev[b];
  Tp = Tp < 0 ? 0 : (Tp > Tcap ? Tcap : Tp);
  if (tid == 0) {
    c_node[0][0] = -1;
    c_last[0][0] = -1;
    c_depth[0][0] = 0;
    c_pb[0][0] = 0.0;
    c_pnb[0][0] = kNinf;
    s_ncur = 1;
    s_err = 0;
  }
  if (tid < k && Tp > 0) {
    cv[0][tid] = topv[tid];
    ci[0][tid] = topi[tid];
  }
  __syncthreads();

  const int pj = tid / kBeam, pi = tid % kBeam;  // pair threads
  int myerr = 0;
  for (int t = 0; t < Tp; ++t) {
    const int cb = t & 1, nb = cb ^ 1;
    const int ncur = s_ncur;
    // next frame's candidates: issued now, written to LDS at the end of the frame
    float nv = 0.f;
    int ni = 0;
    const bool pre = tid < k && t + 1 < Tp;
    if (pre) {
      nv = topv[(int64_t)(t + 1) * k + tid];
      ni = topi[(int64_t)(t + 1) * k + tid];
    }
    // ---- pairs: the extension's slot -------------------------------------------------------
    const bool pair = tid < kPairs && pj < k && pi < ncur;
    int type = 0;  // 0 blank, 1 repeat, 2 extend
    int s = 0, child = -2;
    double ps = 0.0;
    if (pair) {
      s = ci[cb][pj];
      ps = (double)cv[cb][pj];
      const int node = c_node[cb][pi];
      type = s == blank ? 0 : ((node != -1 && s == c_last[cb][pi]) ? 1 : 2);
      if (s < 0) {
        s_err = myerr = E_CAND;  // a row without k finite candidates
      } else if (type != 0) {
        child = child_slot(table, L.table_cap, node, s);
        if (child < 0) {
          s_err = myerr = E_TABLE;
          child = -2;
        }
      }
    }
    if (tid < kPairs) ch[tid] = child;
    __syncthreads();
    // ---- contributions -----------------------------------------------------------------------
    // every thread that forms a field runs the same two log_adds: first {-inf, a1, a2}, then
    // (when a second contribution exists) {first, b1, b2}
    bool has1 = false, has2 = false, owns = false;
    double a1 = kNinf, a2 = kNinf, b1 = kNinf, b2 = kNinf;
    int e_node = 0, e_last = 0, e_depth = 0, key = -1, slot = 0;
    double e_pb = kNinf;
    if (pair && child >= 0) {
      int m = -1;
      for (int q = 0; q < ncur; ++q) m = c_node[cb][q] == child ? q : m;
      if (m < 0) {  // a prefix that is not kept: this pair is its only contribution
        has1 = owns = true;
        a1 = c_pb[cb][pi] + ps;
        a2 = type == 2 ? c_pnb[cb][pi] + ps : kNinf;
        e_node = child;
        e_last = s;
        e_depth = c_depth[cb][pi] + 1;
        key = 2 * tid + (type == 1 ? 1 : 0);
        slot = kBeam + tid;
      }
    } else if (tid >= kPairs && tid < kPairs + kBeam) {  // pb of kept prefix x
      const int x = tid - kPairs;
      int jb = -1;
      for (int j = 0; j < k; ++j) jb = ci[cb][j] == blank ? j : jb;
      if (x < ncur && jb >= 0) {
        has1 = true;
        const double p = (double)cv[cb][jb];
        a1 = c_pb[cb][x] + p;
        a2 = c_pnb[cb][x] + p;
        key = 2 * (jb * kBeam + x);
      }
    } else if (tid >= kPairs + kBeam && tid < kPairs + 2 * kBeam) {  // pnb of kept prefix x
      const int x = tid - kPairs - kBeam;
      if (x < ncur) {
        owns = true;
        slot = x;
        e_node = c_node[cb][x];
        e_last = c_last[cb][x];
        e_depth = c_depth[cb][x];
        int jr = -1;
        if (e_node != -1)
          for (int j = 0; j < k; ++j) jr = ci[cb][j] == e_last ? j : jr;
        if (jr >= 0 && e_last != blank) {
          const double p = (double)cv[cb][jr];
          int ip = -1;  // the kept parent of x
          for (int q = 0; q < ncur; ++q) ip = ch[jr * kBeam + q] == e_node ? q : ip;
          const double r1 = c_pnb[cb][x] + p;  // the repeat of x
          has1 = true;
          key = 2 * (jr * kBeam + x);
          if (ip < 0) {
            a1 = r1;
          } else {
            const bool prep = c_node[cb][ip] != -1 && c_last[cb][ip] == e_last;  // the parent repeats s
            const double x1 = c_pb[cb][ip] + p;
            const double x2 = prep ? kNinf : c_pnb[cb][ip] + p;
            has2 = true;
            if (ip < x) {
              a1 = x1, a2 = x2, b1 = r1;
              key = 2 * (jr * kBeam + ip) + (prep ? 1 : 0);
            } else {
              a1 = r1, b1 = x1, b2 = x2;
            }
          }
        }
      }
    }
    double f = kNinf;
    if (has1) f = log_add3(kNinf, a1, a2);
    if (has2) f = log_add3(f, b1, b2);
    if (tid >= kPairs && tid < kPairs + kBeam) {
      s_pb[tid - kPairs] = f;
      s_pbkey[tid - kPairs] = key;
    }
    __syncthreads();
    // ---- scores ------------------------------------------------------------------------------
    double sc = kNinf;
    if (owns) {
      if (slot < kBeam) {
        e_pb = s_pb[slot];
        const int kb = s_pbkey[slot];
        key = key < 0 ? kb : (kb >= 0 && kb < key ? kb : key);
      }
      if (key >= 0) sc = log_add3(e_pb, f, kNinf);
    }
    if (tid < kPairs) rk[kBeam + tid] = RankKey{sc, (owns && slot >= kBeam) ? key : -1, 0};
    else if (tid >= kPairs + kBeam && tid < kPairs + 2 * kBeam) rk[tid - kPairs - kBeam] = RankKey{sc, owns ? key : -1, 0};
    __syncthreads();
    // ---- rank: entries that come first (score descending, first touch ascending) --------------
    int rank = 0, nvalid = 0;
    for (int q = 0; q < kEnt; ++q) {
      const RankKey o = rk[q];
      const bool valid = o.key >= 0;
      nvalid += valid ? 1 : 0;
      rank += (valid && (o.sc > sc || (o.sc == sc && o.key < key))) ? 1 : 0;
    }
    if (owns && key >= 0 && rank < kBeam) {
      c_node[nb][rank] = e_node;
      c_last[nb][rank] = e_last;
      c_depth[nb][rank] = e_depth;
      c_pb[nb][rank] = e_pb;
      c_pnb[nb][rank] = f;
    }
    if (tid == 0) s_ncur = nvalid < kBeam ? nvalid : kBeam;
    if (pre) {
      cv[nb][tid] = nv;
      ci[nb][tid] = ni;
    }
    // the barrier that ends the frame also agrees on stopping (s_err itself may already be
    // written by a thread that has gone on to the next frame)
    if (__syncthreads_or(myerr)) break;
  }
  __syncthreads();

  // ---- result block ----------------------------------------------------------------------------
  const int fb = Tp & 1;
  const int n = s_err != 0 ? 0 : s_ncur;
  int over = 0;
  if (tid < kBeam) {
    int len = 0;
    double score = kNinf;
    if (tid < n) {
      len = c_depth[fb][tid];
      score = log_add3(c_pb[fb][tid], c_pnb[fb][tid], kNinf);
      if (len > Lcap) {
        over = 1;
      } else {
        int32_t* out = arena + L.toks + (int64_t)tid * Lcap;
        int v = c_node[fb][tid];
        for (int j = len - 1; j >= 0 && v >= 0; --j) {
          const uint64_t kv = ld_l2(table + v);
          out[j] = (int32_t)(uint32_t)kv;
          v = (int32_t)(uint32_t)(kv >> 32);
        }
      }
    }
    arena[R_LENS + tid] = len;
    ((double*)(arena + R_SCORE))[tid] = score;
    ((float*)(arena + R_TOTAL))[tid] = -INFINITY;
  }
  over = __syncthreads_or(over);
  if (tid == 0) {
    arena[R_ERR] = s_err | (over ? E_OVERFLOW : 0);
    arena[R_N] = n;
    arena[R_BEST] = 0;
    arena[R_BESTLEN] = 0;
    arena[R_TP] = Tp;
  }
}

// ---- decoder inputs of the n-best (u2.py:268-298) at the static shape -------------------------
// block (i, q) of grid row b: row q of hypothesis i's decoder mask, its ys_in / gather entry; the
// q = 0 blocks also write the memory mask row: frames >= mem_len[b] masked, or >= the arena's T'
// when mem_len is null.  A hypothesis that overflowed Lcap counts as empty here (the caller runs
// the utterance again), rows >= n are empty.  Utterance b owns hypothesis rows [10 b, 10 b + 10).
__global__ __launch_bounds__(kThreads) void rescore_prep_kernel(const int32_t* __restrict__ arena0, int Tcap, int Lcap,
                                                                int sos, int eos, int32_t* __restrict__ ys_in,
                                                                uint8_t* __restrict__ dec_mask, int dec_ld,
                                                                int32_t* __restrict__ gidx, uint8_t* __restrict__ mem_mask,
                                                                const int32_t* __restrict__ mem_len) {
  const Layout L = make_layout(Tcap, Lcap);
  const int L1 = Lcap + 1;
  const int b = blockIdx.y;
  const int32_t* arena = (const int32_t*)((const char*)arena0 + (int64_t)b * L.total);
  ys_in += (int64_t)b * kBeam * L1;
  dec_mask += (int64_t)b * kBeam * L1 * dec_ld;
  gidx += (int64_t)b * kBeam * L1;
  mem_mask += (int64_t)b * kBeam * Tcap;
  const int i = blockIdx.x / L1, q = blockIdx.x % L1;
  const int n = arena[R_N];
  int len = i < n ? arena[R_LENS + i] : 0;
  if (len > Lcap || len < 0) len = 0;
  const int32_t* tok = arena + L.toks + (int64_t)i * Lcap;
  uint8_t* row = dec_mask + ((int64_t)i * L1 + q) * dec_ld;
  for (int c = threadIdx.x; c < dec_ld; c += kThreads) row[c] = (uint8_t)((c >= L1) || (c >= len + 1) || (c > q));
  if (threadIdx.x == 0) {
    ys_in[(int64_t)i * L1 + q] = q == 0 ? sos : (q - 1 < len ? tok[q - 1] : eos);
    gidx[(int64_t)i * L1 + q] = i < n ? (q < len ? tok[q] : (q == len ? eos : -1)) : -1;
  }
  if (q == 0) {
    const int Tm = mem_len ? mem_len[b] : arena[R_TP];
    for (int t = threadIdx.x; t < Tcap; t += kThreads) mem_mask[(int64_t)i * Tcap + t] = (uint8_t)(t >= Tm);
  }
}

// ---- pick (u2.py:300-315, decoding.pick_best) --------------------------------------------------
// one workgroup per utterance: its arena, its [10][L1cap] block of gathered
__global__ __launch_bounds__(64) void rescore_pick_kernel(int32_t* __restrict__ arena0, int Tcap, int Lcap,
                                                          const float* __restrict__ gathered, double ctc_weight) {
  const Layout L = make_layout(Tcap, Lcap);
  const int L1 = Lcap + 1;
  int32_t* arena = (int32_t*)((char*)arena0 + (int64_t)blockIdx.x * L.total);
  gathered += (int64_t)blockIdx.x * kBeam * L1;
  __shared__ float tot[kBeam];
  __shared__ int s_best;
  const int n = min(max(arena[R_N], 0), kBeam);
  const bool bad = arena[R_ERR] != 0;
  const int tid = threadIdx.x;
  float* gcopy = (float*)(arena + L.gath);
  for (int e = tid; e < kBeam * L1; e += 64) gcopy[e] = gathered[e];
  if (tid < kBeam) {
    float s = -INFINITY;
    if (tid < n && !bad) {
      const int len = min(arena[R_LENS + tid], Lcap);
      s = 0.f;
      for (int j = 0; j <= len; ++j) s = s + gathered[(int64_t)tid * L1 + j];  // tokens, then eos
      s = s + (float)(((const double*)(arena + R_SCORE))[tid] * ctc_weight);
    }
    tot[tid] = s;
    ((float*)(arena + R_TOTAL))[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float best = -INFINITY;
    int bi = 0;
    for (int i = 0; i < n && !bad; ++i)
      if (tot[i] > best) {
        best = tot[i];
        bi = i;
      }
    s_best = bi;
    arena[R_BEST] = bi;
    arena[R_BESTLEN] = (n > 0 && !bad) ? min(arena[R_LENS + bi], Lcap) : 0;
  }
  __syncthreads();
  if (n > 0 && !bad) {
    const int bi = s_best, len = min(arena[R_LENS + bi], Lcap);
    for (int j = tid; j < len; j += 64) arena[L.best + j] = arena[L.toks + (int64_t)bi * Lcap + j];
  }
}

constexpr int kMaxBatch = 4096;

int check_arena(const void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap, const char* who) {
  LASR_CHECK_ARG(arena != nullptr, "%s: null arena", who);
  LASR_CHECK_ARG(B >= 1 && B <= kMaxBatch, "%s: B = %d outside [1, %d]", who, B, kMaxBatch);
  LASR_CHECK_ARG(Tcap >= 1 && Tcap <= (1 << 16), "%s: Tcap = %d outside [1, 65536]", who, Tcap);
  LASR_CHECK_ARG(Lcap >= 1 && Lcap <= (1 << 16), "%s: Lcap = %d outside [1, 65536]", who, Lcap);
  LASR_CHECK_ARG(((uintptr_t)arena & 255) == 0, "%s: arena must be 256-B aligned", who);
  LASR_CHECK_ARG(arena_bytes >= (int64_t)B * make_layout(Tcap, Lcap).total, "%s: arena too small", who);
  return LASR_OK;
}

int search(const char* who, void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap, int k, int blank, int beam,
           const float* topk_val, const int32_t* topk_idx, const int32_t* Tp_dev, void* stream) {
  int rc = check_arena(arena, arena_bytes, B, Tcap, Lcap, who);
  if (rc) return rc;
  LASR_CHECK_ARG(beam == kBeam, "%s: only the reference's beam of 10 is built (got %d)", who, beam);
  LASR_CHECK_ARG(k >= 1 && k <= kBeam, "%s: k = %d outside [1, 10]", who, k);
  LASR_CHECK_ARG(blank >= 0, "%s: blank = %d", who, blank);
  LASR_CHECK_ARG(topk_val && topk_idx && Tp_dev, "%s: null inputs", who);
  const Layout L = make_layout(Tcap, Lcap);
  hipStream_t st = (hipStream_t)stream;
  // table_cap is a power of two >= 1024: two keys per thread, no tail
  const unsigned clear_blocks = (unsigned)(L.table_cap / 2 / 256);
  rescore_clear_kernel<<<dim3(clear_blocks, B), 256, 0, st>>>((char*)arena + L.table, L.total);
  int rc2 = lasr_check_launch("rescore_clear");
  if (rc2) return rc2;
  rescore_search_kernel<<<B, kThreads, 0, st>>>((int32_t*)arena, Tcap, Lcap, k, blank, topk_val, topk_idx, Tp_dev);
  return lasr_check_launch("rescore_search");
}

int prep(const char* who, const void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap, int sos, int eos,
         int32_t* ys_in, uint8_t* dec_mask, int dec_ld, int32_t* gather_idx, uint8_t* mem_mask, const int32_t* mem_len,
         void* stream) {
  int rc = check_arena(arena, arena_bytes, B, Tcap, Lcap, who);
  if (rc) return rc;
  LASR_CHECK_ARG(ys_in && dec_mask && gather_idx && mem_mask, "%s: null outputs", who);
  LASR_CHECK_ARG(dec_ld >= Lcap + 1, "%s: dec_ld = %d < L1cap = %d", who, dec_ld, Lcap + 1);
  LASR_CHECK_ARG(sos >= 0 && eos >= 0, "%s: sos / eos", who);
  rescore_prep_kernel<<<dim3(kBeam * (Lcap + 1), B), kThreads, 0, (hipStream_t)stream>>>(
      (const int32_t*)arena, Tcap, Lcap, sos, eos, ys_in, dec_mask, dec_ld, gather_idx, mem_mask, mem_len);
  return lasr_check_launch("rescore_prep");
}

int pick(const char* who, void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap, const float* gathered,
         double ctc_weight, void* stream) {
  int rc = check_arena(arena, arena_bytes, B, Tcap, Lcap, who);
  if (rc) return rc;
  LASR_CHECK_ARG(gathered != nullptr, "%s: null gathered", who);
  rescore_pick_kernel<<<B, 64, 0, (hipStream_t)stream>>>((int32_t*)arena, Tcap, Lcap, gathered, ctc_weight);
  return lasr_check_launch("rescore_pick");
}

}  // namespace

extern "C" int64_t lasr_rescore_workspace(int Tcap, int Lcap) {
  if (Tcap <= 0 || Lcap <= 0) return 0;
  return make_layout(Tcap, Lcap).total;
}

extern "C" int64_t lasr_rescore_workspace_batch(int B, int Tcap, int Lcap) {
  if (B <= 0 || B > kMaxBatch) return 0;
  return (int64_t)B * lasr_rescore_workspace(Tcap, Lcap);
}

extern "C" int lasr_rescore_search(void* arena, int64_t arena_bytes, int Tcap, int Lcap, int k, int blank, int beam,
                                   const float* topk_val, const int32_t* topk_idx, const int32_t* Tp_dev,
                                   void* stream) {
  return search("lasr_rescore_search", arena, arena_bytes, 1, Tcap, Lcap, k, blank, beam, topk_val, topk_idx, Tp_dev,
                stream);
}

extern "C" int lasr_rescore_search_batch(void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap, int k, int blank,
                                         int beam, const float* topk_val, const int32_t* topk_idx,
                                         const int32_t* Tp_dev, void* stream) {
  return search("lasr_rescore_search_batch", arena, arena_bytes, B, Tcap, Lcap, k, blank, beam, topk_val, topk_idx,
                Tp_dev, stream);
}

extern "C" int lasr_rescore_prep(const void* arena, int64_t arena_bytes, int Tcap, int Lcap, int sos, int eos,
                                 int32_t* ys_in, uint8_t* dec_mask, int dec_ld, int32_t* gather_idx,
                                 uint8_t* mem_mask, void* stream) {
  return prep("lasr_rescore_prep", arena, arena_bytes, 1, Tcap, Lcap, sos, eos, ys_in, dec_mask, dec_ld, gather_idx,
              mem_mask, nullptr, stream);
}

extern "C" int lasr_rescore_prep_batch(const void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap, int sos,
                                       int eos, int32_t* ys_in, uint8_t* dec_mask, int dec_ld, int32_t* gather_idx,
                                       uint8_t* mem_mask, const int32_t* mem_len, void* stream) {
  LASR_CHECK_ARG(mem_len != nullptr, "lasr_rescore_prep_batch: null mem_len");
  return prep("lasr_rescore_prep_batch", arena, arena_bytes, B, Tcap, Lcap, sos, eos, ys_in, dec_mask, dec_ld,
              gather_idx, mem_mask, mem_len, stream);
}

extern "C" int lasr_rescore_pick(void* arena, int64_t arena_bytes, int Tcap, int Lcap, const float* gathered,
                                 double ctc_weight, void* stream) {
  return pick("lasr_rescore_pick", arena, arena_bytes, 1, Tcap, Lcap, gathered, ctc_weight, stream);
}

extern "C" int lasr_rescore_pick_batch(void* arena, int64_t arena_bytes, int B, int Tcap, int Lcap,
                                       const float* gathered, double ctc_weight, void* stream) {
  return pick("lasr_rescore_pick_batch", arena, arena_bytes, B, Tcap, Lcap, gathered, ctc_weight, stream);
}
