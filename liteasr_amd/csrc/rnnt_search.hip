// Transducer beam search on the device (liteasr/models/transducer.py:137-206), SURVEY §8 f4.
//
// The reference's search is a serial chain of batch-1 steps: pop the best hypothesis, one
// LSTM step of the prediction network (memoised by the whole yseq), the tanh joint, a
// log-softmax, top-10, list updates; ten such expansions per encoder frame.  Here the whole
// chain stays on the device.  One expansion is layers + 3 launches:
//
//   step (one per LSTM layer)  fused matvec + LSTMCell gates of hidden unit j per wave, reads
//                              token / parent state through the trie, writes c_j, h_j into
//                              the node's state slot; exits at once when memoised
//   lin_dec                    dec_proj[slot] = lin_dec(h_top), memoised with the state
//   joint                      logits = lin_jnt(tanh(enc_proj[t] + dec_proj[slot]))
//   finalise                   one workgroup: log-sum-exp, the 10 best non-blank log-probs
//                              (descending) + blank, the update of lists A and B with
//                              double scores, child lookup / insert in the trie, and the
//                              selection of the next hypothesis to pop
//
// Hypotheses live in a trie: a node is (parent, token, length, state slot or -1), one node
// per distinct yseq through an open-addressing hash on (parent, token); "memoised by yseq"
// is "the node has a state slot".  A hypothesis is (node, score as double).  List A keeps
// insertion order and marks popped entries dead, so "first maximum in list order" is the
// smallest index among the maxima; it never holds more than 10 + 100 entries per frame.
// Everything is written with plain vector stores by a single workgroup; the launches of a
// stream order the kernels, so no atomics are needed.  Every arena has a capacity; running
// out sets ctrl[ERR] and turns the remaining launches of the utterance into no-ops.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kBeam = 10;
constexpr int kACap = kBeam + kBeam * kBeam;  // physical entries of list A within a frame
constexpr int kThreads = 256;

// ctrl words (int32 unless noted)
enum {
  C_ERR = 0,      // 0 ok, 1 nodes, 2 state slots, 3 hash full, 4 non-finite logits, 5 empty list
  C_POPS = 1,     // expansions finished
  C_TP = 2,       // frames of this utterance
  C_CUR = 3,      // node of the popped hypothesis
  C_DOSTEP = 4,   // its LSTM step is not memoised: the step / lin_dec kernels run
  C_NA = 5,       // physical length of A
  C_ALIVE = 6,    // live entries of A
  C_NB = 7,       // length of B
  C_NNODES = 8,
  C_NSLOTS = 9,
  C_STEPS = 10,   // LSTM steps executed
  C_DONE = 11,    // the last frame is finished: best_* are valid
  C_BEST = 12,    // node of the result
  C_BESTLEN = 13,
  C_CURSCORE = 16,   // double (words 16-17)
  C_BESTSCORE = 18,  // double: score of the result (not normalised)
  C_WORDS = 64,
};

struct Hyp {
  double score;
  int node;
  int alive;
};
struct Node {
  int parent, token, len, slot;
};
struct Pop {
  double score;
  int node, nA;
};

struct Layout {
  int64_t ctrl, cand, yseq, lists, trace, nodes, hash, logits, slots, total;
  int64_t slot_floats, hash_cap;
};

// The documented formula (include/liteasr_hip.h); host and device agree through this one
// function.
__host__ __device__ inline Layout make_layout(int Tcap, int layers, int H, int J, int V, int node_cap, int slot_cap) {
  auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
  Layout L;
  int64_t hc = 64;
  while (hc < 2 * (int64_t)node_cap) hc *= 2;
  L.hash_cap = hc;
  L.slot_floats = ((int64_t)2 * layers * H + J + 63) / 64 * 64;
  int64_t o = 0;
  L.ctrl = o; o += up(C_WORDS * 4);
  L.cand = o; o += up(2 * 16 * 4);
  L.yseq = o; o += up(((int64_t)kBeam * Tcap + 2) * 4);
  L.lists = o; o += up((int64_t)(kACap + kBeam) * 16);
  L.trace = o; o += up((int64_t)kBeam * Tcap * 16);
  L.nodes = o; o += up((int64_t)node_cap * 16);
  L.hash = o; o += up(hc * 4);
  L.logits = o; o += up((int64_t)V * 4);
  L.slots = o; o += up((int64_t)slot_cap * L.slot_floats * 4);
  L.total = o;
  return L;
}

struct View {
  int* ctrl;
  float* candv;
  int* candi;
  int* yseq;
  Hyp* A;
  Hyp* B;
  Pop* trace;
  Node* nodes;
  int* hash;
  float* logits;
  float* slots;
  Layout L;
};

LASR_DEV View make_view(const lasr_rnnt_search_args& a) {
  View v;
  v.L = make_layout(a.Tcap, a.layers, a.H, a.J, a.V, a.node_cap, a.slot_cap);
  char* p = (char*)a.arena;
  v.ctrl = (int*)(p + v.L.ctrl);
  v.candv = (float*)(p + v.L.cand);
  v.candi = (int*)(p + v.L.cand) + 16;
  v.yseq = (int*)(p + v.L.yseq);
  v.A = (Hyp*)(p + v.L.lists);
  v.B = v.A + kACap;
  v.trace = (Pop*)(p + v.L.trace);
  v.nodes = (Node*)(p + v.L.nodes);
  v.hash = (int*)(p + v.L.hash);
  v.logits = (float*)(p + v.L.logits);
  v.slots = (float*)(p + v.L.slots);
  return v;
}

// state slot s: [layers][H] h, [layers][H] c, [J] lin_dec(h_top); all fp32
LASR_DEV float* slot_h(const View& v, const lasr_rnnt_search_args& a, int s, int l) {
  return v.slots + (int64_t)s * v.L.slot_floats + (int64_t)l * a.H;
}
LASR_DEV float* slot_c(const View& v, const lasr_rnnt_search_args& a, int s, int l) {
  return v.slots + (int64_t)s * v.L.slot_floats + (int64_t)(a.layers + l) * a.H;
}
LASR_DEV float* slot_d(const View& v, const lasr_rnnt_search_args& a, int s) {
  return v.slots + (int64_t)s * v.L.slot_floats + (int64_t)2 * a.layers * a.H;
}

LASR_DEV double* dword(int* ctrl, int w) { return (double*)(ctrl + w); }

// ---- wave dot products: NR weight rows (row stride ldw) against one fp32 vector in LDS ----
// 8 columns per lane and trip (16 B of bf16 / 32 B of fp32, coalesced across the wave) when
// the rows allow it, one column per lane otherwise.  Partial sums in a fixed order.
template <typename TW, int NR>
LASR_DEV void wave_dots(const TW* __restrict__ w, int64_t ldw, const float* x, int n, bool vec, float acc[NR]) {
  const int lane = threadIdx.x & 63;
  if (vec) {
    for (int k = lane * 8; k < n; k += 64 * 8) {
      float xv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) xv[q] = x[k + q];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float wv[8];
        ldv<8>(w + r * ldw + k, wv);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[r] = fmaf(wv[q], xv[q], acc[r]);
      }
    }
  } else {
    for (int k = lane; k < n; k += 64) {
      const float xv = x[k];
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[r] = fmaf(to_f(w[r * ldw + k]), xv, acc[r]);
    }
  }
}

template <typename TW>
LASR_DEV bool rows_vec(const TW* w, int n) {
  return n % 8 == 0 && ((uintptr_t)w & 15) == 0;
}

LASR_DEV float sigm_(float x) { return 1.f / (1.f + __expf(-x)); }

// ---- prediction-network step of one layer (rnn_decoder.py:49-64, torch.nn.LSTMCell) -----
// One wave per hidden unit j: the four gate rows i|f|g|o (j, H+j, 2H+j, 3H+j) of W_ih over
// x and of W_hh over h_prev, both biases, then c_j, h_j straight into the node's slot.
template <typename TW>
__global__ __launch_bounds__(kThreads) void search_step_kernel(lasr_rnnt_search_args a, int layer) {
  extern __shared__ float xs[];  // [in] x, then [H] h_prev
  const View v = make_view(a);
  if (v.ctrl[C_ERR] != 0 || v.ctrl[C_DOSTEP] == 0) return;  // memoised (or halted)
  const int H = a.H, in = layer == 0 ? a.dec_dim : H;
  const Node nd = v.nodes[v.ctrl[C_CUR]];
  const int pslot = nd.parent >= 0 ? v.nodes[nd.parent].slot : -1;  // -1: zero state
  const float* x = layer == 0 ? a.embed + (int64_t)nd.token * a.dec_dim : slot_h(v, a, nd.slot, layer - 1);
  const float* hp = pslot >= 0 ? slot_h(v, a, pslot, layer) : nullptr;
  for (int k = threadIdx.x; k < in; k += kThreads) xs[k] = x[k];
  for (int k = threadIdx.x; k < H; k += kThreads) xs[in + k] = hp ? hp[k] : 0.f;
  __syncthreads();
  const int j = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (j >= H) return;
  const TW* Wih = (const TW*)a.Wih[layer] + (int64_t)j * in;
  const TW* Whh = (const TW*)a.Whh[layer] + (int64_t)j * H;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  wave_dots<TW, 4>(Wih, (int64_t)H * in, xs, in, rows_vec((const TW*)a.Wih[layer], in), acc);
  if (hp) wave_dots<TW, 4>(Whh, (int64_t)H * H, xs + in, H, rows_vec((const TW*)a.Whh[layer], H), acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = wave_sum(acc[r]);
  if ((threadIdx.x & 63) == 0) {
    const float* bi = a.bih[layer];
    const float* bh = a.bhh[layer];
    const float ig = sigm_(acc[0] + bi[j] + bh[j]);
    const float fg = sigm_(acc[1] + bi[H + j] + bh[H + j]);
    const float gg = tanhf(acc[2] + bi[2 * H + j] + bh[2 * H + j]);
    const float og = sigm_(acc[3] + bi[3 * H + j] + bh[3 * H + j]);
    const float cp = pslot >= 0 ? slot_c(v, a, pslot, layer)[j] : 0.f;
    const float c = fg * cp + ig * gg;
    slot_c(v, a, nd.slot, layer)[j] = c;
    slot_h(v, a, nd.slot, layer)[j] = og * tanhf(c);
  }
}

// ---- lin_dec of the node's output (transducer.py:222), memoised with the state ----------
template <typename TW>
__global__ __launch_bounds__(kThreads) void search_lin_dec_kernel(lasr_rnnt_search_args a) {
  extern __shared__ float xs[];  // [H]
  const View v = make_view(a);
  if (v.ctrl[C_ERR] != 0 || v.ctrl[C_DOSTEP] == 0) return;
  const int H = a.H, slot = v.nodes[v.ctrl[C_CUR]].slot;
  const float* h = slot_h(v, a, slot, a.layers - 1);
  for (int k = threadIdx.x; k < H; k += kThreads) xs[k] = h[k];
  __syncthreads();
  const int j = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (j >= a.J) return;
  float acc[1] = {0.f};
  wave_dots<TW, 1>((const TW*)a.Wd + (int64_t)j * H, H, xs, H, rows_vec((const TW*)a.Wd, H), acc);
  const float s = wave_sum(acc[0]);
  if ((threadIdx.x & 63) == 0) slot_d(v, a, slot)[j] = s;
}

// ---- joint (transducer.py:220-224): logits = lin_jnt(tanh(enc_proj[t] + dec_proj)) -------
template <typename TW>
__global__ __launch_bounds__(kThreads) void search_joint_kernel(lasr_rnnt_search_args a) {
  extern __shared__ float xs[];  // [J]
  const View v = make_view(a);
  if (v.ctrl[C_ERR] != 0 || v.ctrl[C_DONE] != 0) return;
  const int J = a.J, slot = v.nodes[v.ctrl[C_CUR]].slot;
  const int t = v.ctrl[C_POPS] / kBeam;
  if (slot < 0 || t >= a.Tcap) return;
  const float* e = a.enc_proj + (int64_t)t * J;
  const float* d = slot_d(v, a, slot);
  for (int k = threadIdx.x; k < J; k += kThreads) xs[k] = tanhf(e[k] + d[k]);
  __syncthreads();
  const bool vec = rows_vec((const TW*)a.Wj, J);
  const int nw = gridDim.x * (kThreads / 64);
  for (int c = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); c < a.V; c += nw) {
    float acc[1] = {0.f};
    wave_dots<TW, 1>((const TW*)a.Wj + (int64_t)c * J, J, xs, J, vec, acc);
    const float s = wave_sum(acc[0]);
    if ((threadIdx.x & 63) == 0) v.logits[c] = s + a.bj[c];
  }
}

// ---- trie ---------------------------------------------------------------------------
LASR_DEV uint32_t hash_key(int parent, int token) { return mix32((uint32_t)parent * 0x9E3779B1u ^ mix32((uint32_t)token)); }

// The node of (parent, token): found, or inserted.  -1 with ctrl[ERR] set when an arena is
// full.  Single thread.
LASR_DEV int child_node(const View& v, const lasr_rnnt_search_args& a, int parent, int token) {
  const uint32_t mask = (uint32_t)v.L.hash_cap - 1;
  uint32_t h = hash_key(parent, token) & mask;
  for (int64_t probe = 0; probe < v.L.hash_cap; ++probe, h = (h + 1) & mask) {
    const int n = v.hash[h];
    if (n < 0) {
      const int id = v.ctrl[C_NNODES];
      if (id >= a.node_cap) {
        v.ctrl[C_ERR] = 1;
        return -1;
      }
      v.ctrl[C_NNODES] = id + 1;
      v.nodes[id] = Node{parent, token, v.nodes[parent].len + 1, -1};
      v.hash[h] = id;
      return id;
    }
    if (v.nodes[n].parent == parent && v.nodes[n].token == token) return n;
  }
  v.ctrl[C_ERR] = 3;
  return -1;
}

// Pop the best live hypothesis of A (first index among the maxima), record it, and give its
// node a state slot when its step is not memoised yet.  Called by the first wave.
LASR_DEV void select_next(const View& v, const lasr_rnnt_search_args& a) {
  const int lane = threadIdx.x & 63;
  const int nA = v.ctrl[C_NA];
  double bs = 0.0;
  int bi = 0x7fffffff;
  for (int i = lane; i < nA; i += 64) {
    const Hyp h = v.A[i];
    if (h.alive && (bi == 0x7fffffff || h.score > bs)) {
      bs = h.score;
      bi = i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(bs, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || os > bs || (os == bs && oi < bi))) {
      bs = os;
      bi = oi;
    }
  }
  if (lane != 0) return;
  if (bi == 0x7fffffff) {
    v.ctrl[C_ERR] = 5;
    v.ctrl[C_DOSTEP] = 0;
    return;
  }
  const int pops = v.ctrl[C_POPS];
  const int node = v.A[bi].node;
  v.trace[pops] = Pop{bs, node, v.ctrl[C_ALIVE]};
  v.A[bi].alive = 0;
  v.ctrl[C_ALIVE] -= 1;
  v.ctrl[C_CUR] = node;
  *dword(v.ctrl, C_CURSCORE) = bs;
  int dostep = 0;
  if (v.nodes[node].slot < 0) {
    const int s = v.ctrl[C_NSLOTS];
    if (s >= a.slot_cap) {
      v.ctrl[C_ERR] = 2;
    } else {
      v.ctrl[C_NSLOTS] = s + 1;
      v.nodes[node].slot = s;
      v.ctrl[C_STEPS] += 1;
      dostep = 1;
    }
  }
  v.ctrl[C_DOSTEP] = dostep;
}

// ---- start of an utterance: empty trie, root hypothesis popped ------------------------
__global__ __launch_bounds__(kThreads) void search_init_kernel(lasr_rnnt_search_args a, int Tp) {
  const View v = make_view(a);
  for (int64_t i = threadIdx.x; i < v.L.hash_cap; i += kThreads) v.hash[i] = -1;
  for (int i = threadIdx.x; i < C_WORDS; i += kThreads) v.ctrl[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    v.ctrl[C_TP] = Tp;
    v.ctrl[C_NNODES] = 1;
    v.ctrl[C_NA] = 1;
    v.ctrl[C_ALIVE] = 1;
    v.nodes[0] = Node{-1, 0, 1, -1};  // yseq [0]
    v.A[0] = Hyp{0.0, 0, 1};
  }
  __syncthreads();
  if (threadIdx.x < 64) select_next(v, a);
}

// ---- finalise one expansion ------------------------------------------------------------
// mode 0: the whole search step.  mode 1 (host-loop driver, tests and tools): stop after the
// candidates (log-probs of blank + the 10 best non-blank tokens).
__global__ __launch_bounds__(kThreads) void search_finalise_kernel(lasr_rnnt_search_args a, int mode) {
  extern __shared__ float row[];  // [V]
  __shared__ float red[16];
  __shared__ float redv[16];
  __shared__ int redi[16];
  const View v = make_view(a);
  if (v.ctrl[C_ERR] != 0 || v.ctrl[C_DONE] != 0) return;
  if (v.nodes[v.ctrl[C_CUR]].slot < 0) return;
  const int V = a.V;
  float m = -INFINITY;
  for (int c = threadIdx.x; c < V; c += kThreads) {
    const float x = v.logits[c];
    row[c] = x;
    m = fmaxf(m, x);
  }
  m = block_max(m, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += kThreads) s += __expf(row[c] - m);
  s = block_sum(s, red);
  const float lse = logf(s);
  if (threadIdx.x == 0) {
    v.candv[kBeam] = (row[0] - m) - lse;  // blank last, as the reference's torch.cat
    v.candi[kBeam] = 0;
    row[0] = -INFINITY;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int j = 0; j < kBeam; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    __syncthreads();  // row[] masked by the previous round
    for (int c = threadIdx.x; c < V; c += kThreads) {
      const float x = row[c];
      if (x > bv || (x == bv && c < bi)) {
        bv = x;
        bi = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      redv[w] = bv;
      redi[w] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 1; i < kThreads / 64; ++i)
        if (redv[i] > bv || (redv[i] == bv && redi[i] < bi)) {
          bv = redv[i];
          bi = redi[i];
        }
      if (bi >= V) {  // NaN logits: nothing compares
        v.ctrl[C_ERR] = 4;
        bi = 1;
      }
      v.candv[j] = (bv - m) - lse;
      v.candi[j] = bi;
      row[bi] = -INFINITY;
    }
  }
  __syncthreads();
  if (mode != 0 || threadIdx.x >= 64 || v.ctrl[C_ERR] != 0) return;
  // list updates (transducer.py:174-201), one thread; the candidates just written are read
  // back by the thread that wrote them
  int frame_done = 0;
  if (threadIdx.x == 0) {
    const int cur = v.ctrl[C_CUR];
    const double sc = *dword(v.ctrl, C_CURSCORE);
    int nA = v.ctrl[C_NA];
    for (int j = 0; j < kBeam; ++j) {
      const int ch = child_node(v, a, cur, v.candi[j]);
      if (ch < 0) break;
      v.A[nA++] = Hyp{sc + (double)v.candv[j], ch, 1};
    }
    if (v.ctrl[C_ERR] == 0) {
      v.ctrl[C_NA] = nA;
      v.ctrl[C_ALIVE] += kBeam;
      int nB = v.ctrl[C_NB];
      v.B[nB++] = Hyp{sc + (double)v.candv[kBeam], cur, 1};
      const int pops = v.ctrl[C_POPS] + 1;
      v.ctrl[C_POPS] = pops;
      if (nB >= kBeam) {  // the frame is finished: kept = B
        frame_done = 1;
        for (int i = 0; i < kBeam; ++i) v.A[i] = v.B[i];
        v.ctrl[C_NA] = kBeam;
        v.ctrl[C_ALIVE] = kBeam;
        nB = 0;
        if (pops >= kBeam * v.ctrl[C_TP]) {
          // transducer.py:203-206: first maximum of score / len(yseq)
          int best = 0;
          double bn = v.B[0].score / v.nodes[v.B[0].node].len;
          for (int i = 1; i < kBeam; ++i) {
            const double n = v.B[i].score / v.nodes[v.B[i].node].len;
            if (n > bn) {
              bn = n;
              best = i;
            }
          }
          int node = v.B[best].node;
          const int len = v.nodes[node].len;
          v.ctrl[C_BEST] = node;
          v.ctrl[C_BESTLEN] = len;
          *dword(v.ctrl, C_BESTSCORE) = v.B[best].score;
          for (int i = len - 1; i >= 0 && node >= 0; --i, node = v.nodes[node].parent) v.yseq[i] = v.nodes[node].token;
          v.ctrl[C_DONE] = 1;
          frame_done = 2;
        }
      }
      v.ctrl[C_NB] = nB;
    } else {
      frame_done = 2;
    }
  }
  frame_done = __shfl(frame_done, 0, 64);
  if (frame_done == 2) return;
  __threadfence_block();
  select_next(v, a);
}

int check_args(const lasr_rnnt_search_args* a, const char* who) {
  LASR_CHECK_ARG(a != nullptr && a->arena != nullptr, "%s: null arguments", who);
  LASR_CHECK_ARG(a->Tcap > 0 && a->layers > 0 && a->layers <= LASR_RNNT_SEARCH_MAX_LAYERS && a->dec_dim > 0 &&
                     a->H > 0 && a->J > 0,
                 "%s: bad sizes", who);
  LASR_CHECK_ARG(a->V >= kBeam + 1 && a->V <= 16000, "%s: V = %d outside [11, 16000]", who, a->V);
  LASR_CHECK_ARG(a->node_cap >= 1 && a->slot_cap >= 1, "%s: capacities must be positive", who);
  LASR_CHECK_ARG(a->w_dtype == LASR_F32 || a->w_dtype == LASR_BF16, "%s: bad weight dtype", who);
  LASR_CHECK_ARG((int64_t)(a->dec_dim + a->H) * 4 <= 64 * 1024 && (int64_t)a->J * 4 <= 64 * 1024,
                 "%s: dec_dim + H or J too large for the LDS staging", who);
  LASR_CHECK_ARG(a->arena_bytes >= lasr_rnnt_search_workspace(a->Tcap, a->layers, a->H, a->J, a->V, a->node_cap,
                                                              a->slot_cap),
                 "%s: arena too small", who);
  LASR_CHECK_ARG(((uintptr_t)a->arena & 255) == 0, "%s: arena must be 256-B aligned", who);
  LASR_CHECK_ARG(a->embed && a->Wd && a->Wj && a->bj && a->enc_proj, "%s: null weights", who);
  for (int l = 0; l < a->layers; ++l)
    LASR_CHECK_ARG(a->Wih[l] && a->Whh[l] && a->bih[l] && a->bhh[l], "%s: null LSTM weights (layer %d)", who, l);
  return LASR_OK;
}

}  // namespace

extern "C" int64_t lasr_rnnt_search_workspace(int Tcap, int layers, int H, int J, int V, int node_cap, int slot_cap) {
  if (Tcap <= 0 || layers <= 0 || H <= 0 || J <= 0 || V <= 0) return 0;
  if (node_cap <= 0) node_cap = kBeam * kBeam * Tcap + 1;
  if (slot_cap <= 0) slot_cap = kBeam * Tcap + 1;
  return make_layout(Tcap, layers, H, J, V, node_cap, slot_cap).total;
}

extern "C" int lasr_rnnt_search_init(const lasr_rnnt_search_args* a, int Tp, void* stream) {
  int rc = check_args(a, "lasr_rnnt_search_init");
  if (rc) return rc;
  LASR_CHECK_ARG(Tp > 0 && Tp <= a->Tcap, "lasr_rnnt_search_init: T' = %d outside [1, Tcap = %d]", Tp, a->Tcap);
  search_init_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(*a, Tp);
  return lasr_check_launch("rnnt_search_init");
}

extern "C" int lasr_rnnt_search_expand(const lasr_rnnt_search_args* a, int mode, void* stream) {
  int rc = check_args(a, "lasr_rnnt_search_expand");
  if (rc) return rc;
  LASR_CHECK_ARG(mode == 0 || mode == 1, "lasr_rnnt_search_expand: mode %d", mode);
  hipStream_t st = (hipStream_t)stream;
  const int wpb = kThreads / 64;
  const unsigned gh = (unsigned)cdiv(a->H, wpb), gj = (unsigned)cdiv(a->J, wpb);
  const unsigned gv = (unsigned)std::min<int64_t>(cdiv(a->V, wpb), 2048);
#define SEARCH_CHAIN(TW)                                                                                  \
  do {                                                                                                    \
    for (int l = 0; l < a->layers; ++l) {                                                                 \
      const size_t lds = (size_t)((l == 0 ? a->dec_dim : a->H) + a->H) * sizeof(float);                   \
      search_step_kernel<TW><<<gh, kThreads, lds, st>>>(*a, l);                                           \
    }                                                                                                     \
    search_lin_dec_kernel<TW><<<gj, kThreads, (size_t)a->H * sizeof(float), st>>>(*a);                    \
    search_joint_kernel<TW><<<gv, kThreads, (size_t)a->J * sizeof(float), st>>>(*a);                      \
  } while (0)
  if (a->w_dtype == LASR_F32) SEARCH_CHAIN(float);
  else SEARCH_CHAIN(bf16_t);
#undef SEARCH_CHAIN
  rc = lasr_check_launch("rnnt_search_chain");
  if (rc) return rc;
  search_finalise_kernel<<<1, kThreads, (size_t)a->V * sizeof(float), st>>>(*a, mode);
  return lasr_check_launch("rnnt_search_finalise");
}
