// wav2vec 2.0 pretraining kernels (liteasr/models/wav2vec2.py and the nets it builds on):
// the feature extractor's first layer and its fused LayerNorm + GELU, the col2im add of the
// strided-view convolution GEMMs, the grouped positional convolution's layout kernels, the mask
// embedding, the Gumbel vector quantizer and the contrastive head.  Every reduction here runs
// in a fixed order (no floating-point atomics): two runs give the same bits.
#include "common.h"

namespace {

constexpr int W2V_KMAX = 16;      // layer-0 kernel width limit (taps kept in registers)
constexpr int W2V_LN_ROWS = 64;   // rows per block of the LN + GELU backward (4 waves x 16)
constexpr float W2V_COS_EPS = 1e-8f;  // torch.cosine_similarity's eps

LASR_DEV float ldx(const void* p, int dt, int64_t i) {
  return dt == LASR_F32 ? ((const float*)p)[i] : bf2f(((const bf16_t*)p)[i]);
}
LASR_DEV void stx(void* p, int dt, int64_t i, float v) {
  if (dt == LASR_F32) ((float*)p)[i] = v;
  else ((bf16_t*)p)[i] = f2bf(v);
}
// exact (erf) GELU and its derivative (torch.nn.GELU default)
LASR_DEV float gelu_f(float u) { return 0.5f * u * (1.f + erff(u * 0.70710678118654752f)); }
LASR_DEV float gelu_g(float u) {
  return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * 0.39894228040143268f * expf(-0.5f * u * u);
}
inline unsigned grid1(int64_t n, int bs = 256) { return (unsigned)cdiv(n, bs); }
inline bool dt_ok(int dt) { return dt == LASR_F32 || dt == LASR_BF16; }

// ------------------------------------------------------------- extractor layer 0
// y[b, t, c] = bias[c] + sum_j w[c, j] x[b, s t + j]   (C_in = 1)
__global__ void conv0_fwd_kernel(const float* __restrict__ x, int B, int Tin, int Tout, int C, int k, int s,
                                 const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * Tout * C) return;
  const int c = (int)(i % C);
  const int64_t r = i / C;
  const int t = (int)(r % Tout), b = (int)(r / Tout);
  const float* xr = x + (int64_t)b * Tin + (int64_t)s * t;
  float acc = bias ? bias[c] : 0.f;
  for (int j = 0; j < k; ++j) acc += w[c * k + j] * xr[j];
  y[i] = acc;
}

// part[p][c k + j] = sum over the rows of chunk p of dy[r, c] x[b, s t + j]; block (64, 4)
__global__ void conv0_dw_kernel(const float* __restrict__ x, const void* __restrict__ dy, int dydt, int B, int Tin,
                                int Tout, int C, int k, int s, int64_t chunk, float* __restrict__ part) {
  __shared__ float sm[4][64][W2V_KMAX + 1];
  const int cx = threadIdx.x, ty = threadIdx.y;
  const int c = blockIdx.x * 64 + cx;
  const int64_t rows = (int64_t)B * Tout;
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  float acc[W2V_KMAX];
#pragma unroll
  for (int j = 0; j < W2V_KMAX; ++j) acc[j] = 0.f;
  if (c < C) {
    for (int64_t r = r0 + ty; r < r1; r += 4) {
      const int t = (int)(r % Tout), b = (int)(r / Tout);
      const float g = ldx(dy, dydt, r * C + c);
      const float* xr = x + (int64_t)b * Tin + (int64_t)s * t;
#pragma unroll
      for (int j = 0; j < W2V_KMAX; ++j)
        if (j < k) acc[j] += g * xr[j];
    }
  }
#pragma unroll
  for (int j = 0; j < W2V_KMAX; ++j) sm[ty][cx][j] = acc[j];
  __syncthreads();
  if (ty == 0 && c < C) {
    for (int j = 0; j < k; ++j)
      part[(int64_t)blockIdx.y * C * k + (int64_t)c * k + j] = sm[0][cx][j] + sm[1][cx][j] + sm[2][cx][j] + sm[3][cx][j];
  }
}

// ------------------------------------------------------ LayerNorm (+ GELU), fp32 statistics
// one wave per row; y = act(xhat gamma + beta)
__global__ void ln_act_fwd_kernel(const void* __restrict__ x, int xdt, int64_t rows, int C,
                                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int act,
                                  void* __restrict__ y, int ydt, float* __restrict__ mean, float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t o = r * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += ldx(x, xdt, o + c);
  const float mu = wave_sum(s) / (float)C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = ldx(x, xdt, o + c) - mu;
    v += d * d;
  }
  const float rs = 1.f / sqrtf(wave_sum(v) / (float)C + eps);
  for (int c = lane; c < C; c += 64) {
    const float u = (ldx(x, xdt, o + c) - mu) * rs * gamma[c] + beta[c];
    stx(y, ydt, o + c, act ? gelu_f(u) : u);
  }
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// block = 4 waves x 16 rows; dynamic LDS [4][2][C]: each wave's own gamma / beta partials
__global__ void ln_act_bwd_kernel(const void* __restrict__ x, int xdt, const void* __restrict__ dy, int dydt,
                                  int64_t rows, int C, const float* __restrict__ gamma,
                                  const float* __restrict__ beta, const float* __restrict__ mean,
                                  const float* __restrict__ rstd, int act, void* __restrict__ dx, int dxdt,
                                  float* __restrict__ part) {
  extern __shared__ float sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* sg = sm + (int64_t)w * 2 * C;
  float* sb = sg + C;
  for (int c = lane; c < C; c += 64) sg[c] = sb[c] = 0.f;
  const int64_t base = (int64_t)blockIdx.x * W2V_LN_ROWS;
  for (int i = 0; i < W2V_LN_ROWS / 4; ++i) {
    const int64_t r = base + w + 4 * i;
    if (r >= rows) break;
    const int64_t o = r * C;
    const float mu = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float xh = (ldx(x, xdt, o + c) - mu) * rs;
      float g = ldx(dy, dydt, o + c);
      if (act) g *= gelu_g(xh * gamma[c] + beta[c]);
      sg[c] += g * xh;
      sb[c] += g;
      const float dxh = g * gamma[c];
      s1 += dxh;
      s2 += dxh * xh;
    }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)C;
    for (int c = lane; c < C; c += 64) {
      const float xh = (ldx(x, xdt, o + c) - mu) * rs;
      float g = ldx(dy, dydt, o + c);
      if (act) g *= gelu_g(xh * gamma[c] + beta[c]);
      stx(dx, dxdt, o + c, rs * (g * gamma[c] - s1 - xh * s2));
    }
  }
  __syncthreads();
  float* pr = part + (int64_t)blockIdx.x * 2 * C;
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x)
    pr[c] = sm[c] + sm[2 * C + c] + sm[4 * C + c] + sm[6 * C + c];
}

// ------------------------------------------------------------------ col2im (1-D)
// dx[b, ti, c] = sum over (t, j) with s t + j == ti of dcol[b, t, j C + c], j ascending
__global__ void col2im1d_kernel(const void* __restrict__ dcol, int dt, int B, int Tin, int Tout, int C, int k, int s,
                                float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * Tin * C) return;
  const int c = (int)(i % C);
  const int64_t r = i / C;
  const int ti = (int)(r % Tin), b = (int)(r / Tin);
  float acc = 0.f;
  for (int j = 0; j < k; ++j) {
    const int q = ti - j;
    if (q < 0 || q % s) continue;
    const int t = q / s;
    if (t < Tout) acc += ldx(dcol, dt, ((int64_t)b * Tout + t) * k * C + (int64_t)j * C + c);
  }
  dx[i] = acc;
}

// ------------------------------------------------- grouped positional convolution
// dst[g][b][u][c] (u < Tp) = src[b][u - front][g cg + c] (0 outside), times
// GELU'(yg[g][b][t][c] + bias) when yg is given (the backward's dY)
__global__ void group_pack_kernel(const float* __restrict__ src, int B, int T, int G, int cg, int front, int Tp,
                                  const void* __restrict__ yg, int ygdt, const float* __restrict__ bias,
                                  void* __restrict__ dst, int ddt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)G * B * Tp * cg) return;
  const int c = (int)(i % cg);
  int64_t r = i / cg;
  const int u = (int)(r % Tp);
  r /= Tp;
  const int b = (int)(r % B), g = (int)(r / B);
  const int t = u - front;
  float v = 0.f;
  if (t >= 0 && t < T) {
    v = src[((int64_t)b * T + t) * G * cg + g * cg + c];
    if (yg) v *= gelu_g(ldx(yg, ygdt, (((int64_t)g * B + b) * T + t) * cg + c) + (bias ? bias[g * cg + c] : 0.f));
  }
  stx(dst, ddt, i, v);
}

// out[b][t][g cg + c] = res + act(yg[g][b][t][c] + bias)
__global__ void group_unpack_kernel(const void* __restrict__ yg, int ygdt, const float* __restrict__ bias, int act,
                                    const float* __restrict__ res, int B, int T, int G, int cg,
                                    float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int d = G * cg;
  if (i >= (int64_t)B * T * d) return;
  const int ch = (int)(i % d);
  const int64_t r = i / d;
  const int t = (int)(r % T), b = (int)(r / T);
  const int g = ch / cg, c = ch % cg;
  float v = ldx(yg, ygdt, (((int64_t)g * B + b) * T + t) * cg + c) + (bias ? bias[ch] : 0.f);
  if (act) v = gelu_f(v);
  out[i] = (res ? res[i] : 0.f) + v;
}

// out[g cg + c] += sum over the rows of x[g][rows][cg]; one block per channel
__global__ void group_colsum_kernel(const void* __restrict__ x, int dt, int64_t rows, int cg, float* __restrict__ out) {
  __shared__ float red[16];
  const int ch = blockIdx.x, g = ch / cg, c = ch % cg;
  float acc = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += blockDim.x) acc += ldx(x, dt, ((int64_t)g * rows + r) * cg + c);
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[ch] += acc;
}

// ------------------------------------------------------------------ mask / gather
__global__ void mask_fwd_kernel(float* __restrict__ x, const int32_t* __restrict__ midx, int B, int T, int M, int d,
                                const float* __restrict__ emb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * M * d) return;
  const int c = (int)(i % d);
  const int64_t r = i / d;
  const int b = (int)(r / M);
  const int t = midx[r];
  if (t < 0 || t >= T) return;
  x[((int64_t)b * T + t) * d + c] = emb[c];
}

// one thread per channel walks the masked rows in (b, m) order: demb += dx[row], dx[row] = 0
__global__ void mask_bwd_kernel(float* __restrict__ dx, const int32_t* __restrict__ midx, int B, int T, int M, int d,
                                float* __restrict__ demb) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d) return;
  float acc = 0.f;
  for (int r = 0; r < B * M; ++r) {
    const int t = midx[r];
    if (t < 0 || t >= T) continue;
    const int64_t o = ((int64_t)(r / M) * T + t) * d + c;
    acc += dx[o];
    dx[o] = 0.f;
  }
  demb[c] += acc;
}

__global__ void gather_rows_kernel(const void* __restrict__ src, int sdt, int64_t sb, int64_t st,
                                   const int32_t* __restrict__ midx, int B, int T, int M, int d,
                                   void* __restrict__ dst, int ddt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * M * d) return;
  const int c = (int)(i % d);
  const int64_t r = i / d;
  const int b = (int)(r / M);
  const int t = midx[r];
  stx(dst, ddt, i, (t >= 0 && t < T) ? ldx(src, sdt, b * sb + t * st + c) : 0.f);
}

__global__ void scatter_rows_kernel(const void* __restrict__ src, int sdt, const int32_t* __restrict__ midx, int B,
                                    int T, int M, int d, float* __restrict__ dst, int64_t sb, int64_t st,
                                    int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * M * d) return;
  const int c = (int)(i % d);
  const int64_t r = i / d;
  const int b = (int)(r / M);
  const int t = midx[r];
  if (t < 0 || t >= T) return;
  const int64_t o = b * sb + t * st + c;
  const float v = ldx(src, sdt, i);
  dst[o] = accumulate ? dst[o] + v : v;
}

// ------------------------------------------------------- Gumbel vector quantizer
// standard Gumbel draw of element idx from the library's counter hash (24 bits, u in (0, 1))
LASR_DEV float gumbel_draw(uint32_t key, uint64_t idx) {
  const float u = ((float)(drop_bits(key, idx) >> 8) + 0.5f) * (1.f / 16777216.f);
  return -logf(-logf(u));
}
LASR_DEV float gumbel_z(const void* lg, int dt, const float* noise, uint32_t key, int64_t i, float inv_tau,
                        int hard) {
  const float l = ldx(lg, dt, i);
  if (hard) return l;
  return (l + (noise ? noise[i] : gumbel_draw(key, (uint64_t)i))) * inv_tau;
}

// one wave per (row, group): code = argmax z (ties: the smaller index), out = vars[code]
__global__ void gumbel_fwd_kernel(const void* __restrict__ lg, int dt, const float* __restrict__ noise, DropCfg dc,
                                  float inv_tau, int hard, int64_t RG, int G, int V, const float* __restrict__ vars,
                                  int vd, void* __restrict__ out, int odt, int32_t* __restrict__ codes) {
  const int lane = threadIdx.x & 63;
  const int64_t rg = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (rg >= RG) return;
  const uint32_t key = (hard || noise) ? 0u : drop_key(dc);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float z = gumbel_z(lg, dt, noise, key, rg * V + v, inv_tau, hard);
    if (z > best || (z == best && v < bi)) {
      best = z;
      bi = v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (bi >= V) bi = 0;  // a row of NaNs
  const int g = (int)(rg % G);
  if (lane == 0) codes[rg] = bi;
  const float* vr = vars + ((int64_t)g * V + bi) * vd;
  for (int c = lane; c < vd; c += 64) stx(out, odt, rg * vd + c, vr[c]);
}

// one wave (= block) per (row, group): dlogit = y (s - <y, s>) / tau, y = softmax(z),
// s_v = <dout[row, group], vars[group, v]>; LDS: s [V]
__global__ void gumbel_bwd_kernel(const void* __restrict__ lg, int dt, const float* __restrict__ noise, DropCfg dc,
                                  float inv_tau, int G, int V, const float* __restrict__ vars, int vd,
                                  const void* __restrict__ dout, int dodt, void* __restrict__ dlg, int dldt) {
  extern __shared__ float sh[];
  const int lane = threadIdx.x;
  const int64_t rg = blockIdx.x;
  const int g = (int)(rg % G);
  const uint32_t key = noise ? 0u : drop_key(dc);
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, gumbel_z(lg, dt, noise, key, rg * V + v, inv_tau, 0));
  mx = wave_max(mx);
  float se = 0.f, ys = 0.f;
  for (int v = lane; v < V; v += 64) {
    const float e = expf(gumbel_z(lg, dt, noise, key, rg * V + v, inv_tau, 0) - mx);
    const float* vr = vars + ((int64_t)g * V + v) * vd;
    float s = 0.f;
    for (int c = 0; c < vd; ++c) s += ldx(dout, dodt, rg * vd + c) * vr[c];
    sh[v] = s;
    se += e;
    ys += e * s;
  }
  se = wave_sum(se);
  ys = wave_sum(ys) / se;
  for (int v = lane; v < V; v += 64) {
    const float y = expf(gumbel_z(lg, dt, noise, key, rg * V + v, inv_tau, 0) - mx) / se;
    stx(dlg, dldt, rg * V + v, y * (sh[v] - ys) * inv_tau);
  }
}

// dvars[g V + v] += sum, rows ascending, of dout[r, g] over the rows that chose code v; block per (g, v)
__global__ void gumbel_dvars_kernel(const int32_t* __restrict__ codes, int64_t R, int G, int V, int vd,
                                    const void* __restrict__ dout, int dodt, float* __restrict__ dvars) {
  const int gv = blockIdx.x, g = gv / V, v = gv % V;
  for (int c = threadIdx.x; c < vd; c += blockDim.x) {
    float acc = 0.f;
    for (int64_t r = 0; r < R; ++r)
      if (codes[r * G + g] == v) acc += ldx(dout, dodt, (r * G + g) * vd + c);
    dvars[(int64_t)gv * vd + c] += acc;
  }
}

// ------------------------------------------------------------- contrastive head
struct CosRow {
  float dot, nt;
};
LASR_DEV CosRow cos_row(const float* __restrict__ x, const float* __restrict__ t, int D, int lane) {
  float d = 0.f, n = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float tv = t[c];
    d += x[c] * tv;
    n += tv * tv;
  }
  CosRow r;
  r.dot = wave_sum(d);
  r.nt = sqrtf(wave_sum(n));
  return r;
}
LASR_DEV bool same_codes(const int32_t* codes, int G, int64_t a, int64_t b) {
  for (int g = 0; g < G; ++g)
    if (codes[a * G + g] != codes[b * G + g]) return false;
  return true;
}

// one wave (= block) per (b, m): logits row m B + b, its log-sum-exp and cross-entropy vs class 0
__global__ void contrast_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                    const int32_t* __restrict__ neg, const int32_t* __restrict__ codes, int G, int B,
                                    int M, int N, int D, float inv_temp, float* __restrict__ logits,
                                    float* __restrict__ lse, float* __restrict__ row_loss) {
  extern __shared__ float sh[];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;  // b M + m
  const int b = (int)(row / M), m = (int)(row % M);
  const float* xr = x + row * D;
  float nx = 0.f;
  for (int c = lane; c < D; c += 64) nx += xr[c] * xr[c];
  nx = fmaxf(sqrtf(wave_sum(nx)), W2V_COS_EPS);
  const int64_t orow = ((int64_t)m * B + b) * (N + 1);
  for (int n = 0; n <= N; ++n) {
    const int64_t j = n == 0 ? row : (int64_t)neg[row * N + n - 1];
    float lgt = -INFINITY;
    if (j >= 0 && j < (int64_t)B * M && !(n > 0 && same_codes(codes, G, j, row))) {
      const CosRow cr = cos_row(xr, y + j * D, D, lane);
      lgt = cr.dot / (nx * fmaxf(cr.nt, W2V_COS_EPS)) * inv_temp;
    }
    if (lane == 0) {
      sh[n] = lgt;
      logits[orow + n] = lgt;
    }
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int n = lane; n <= N; n += 64) mx = fmaxf(mx, sh[n]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int n = lane; n <= N; n += 64) se += expf(sh[n] - mx);
  se = wave_sum(se);
  if (lane == 0) {
    const float l = mx + logf(se);
    lse[row] = l;
    row_loss[row] = l - sh[0];
  }
}

__global__ void mean_kernel(const float* __restrict__ v, int64_t n, float* __restrict__ out) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) acc += v[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = acc / (float)n;
}

// pass A, one wave per (b, m): the row's softmax gradient, dx, and per target the two
// coefficients pass B needs: dt = ca x - cc t
__global__ void contrast_bwd_x_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                      const int32_t* __restrict__ neg, const int32_t* __restrict__ codes, int G,
                                      int B, int M, int N, int D, float inv_temp, const float* __restrict__ lse,
                                      const float* __restrict__ gout, float* __restrict__ dx,
                                      float* __restrict__ coef) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* xr = x + row * D;
  float* dxr = dx + row * D;
  float nx2 = 0.f;
  for (int c = lane; c < D; c += 64) {
    nx2 += xr[c] * xr[c];
    dxr[c] = 0.f;
  }
  nx2 = wave_sum(nx2);
  const float nxr = sqrtf(nx2), nx = fmaxf(nxr, W2V_COS_EPS);
  const float gs = (gout ? gout[0] : 1.f) / (float)((int64_t)B * M);
  const float l = lse[row];
  float self = 0.f;  // sum_n dcos_n cos_n
  for (int n = 0; n <= N; ++n) {
    const int64_t j = n == 0 ? row : (int64_t)neg[row * N + n - 1];
    float ca = 0.f, cc = 0.f;
    if (j >= 0 && j < (int64_t)B * M && !(n > 0 && same_codes(codes, G, j, row))) {
      const float* tr = y + j * D;
      const CosRow cr = cos_row(xr, tr, D, lane);
      const float nt = fmaxf(cr.nt, W2V_COS_EPS);
      const float cs = cr.dot / (nx * nt);
      const float dcos = gs * (expf(cs * inv_temp - l) - (n == 0 ? 1.f : 0.f)) * inv_temp;
      ca = dcos / (nx * nt);
      cc = cr.nt > W2V_COS_EPS ? dcos * cs / (nt * nt) : 0.f;
      self += dcos * cs;
      for (int c = lane; c < D; c += 64) dxr[c] += ca * tr[c];
    }
    if (lane == 0) {
      coef[(row * (N + 1) + n) * 2] = ca;
      coef[(row * (N + 1) + n) * 2 + 1] = cc;
    }
  }
  if (nxr > W2V_COS_EPS) {
    const float k = self / nx2;
    for (int c = lane; c < D; c += 64) dxr[c] -= k * xr[c];
  }
}

// pass B, one wave per target row j = (b, mj): the positive's term, then every (m, n) of the
// utterance whose index points at j, in (m, n) order
__global__ void contrast_bwd_y_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                      const int32_t* __restrict__ neg, int B, int M, int N, int D,
                                      const float* __restrict__ coef, float* __restrict__ dy) {
  const int lane = threadIdx.x;
  const int64_t j = blockIdx.x;
  const int b = (int)(j / M);
  const float* yr = y + j * D;
  float* dyr = dy + j * D;
  {
    const float ca = coef[(j * (N + 1)) * 2], cc = coef[(j * (N + 1)) * 2 + 1];
    for (int c = lane; c < D; c += 64) dyr[c] = ca * x[j * D + c] - cc * yr[c];
  }
  const int64_t E = (int64_t)M * N;
  const int32_t* nb = neg + (int64_t)b * E;
  for (int64_t e0 = 0; e0 < E; e0 += 64) {
    const int64_t e = e0 + lane;
    unsigned long long hits = __ballot(e < E && (int64_t)nb[e] == j);
    while (hits) {
      const int k = __ffsll((long long)hits) - 1;
      hits &= hits - 1;
      const int64_t ee = e0 + k;
      const int64_t row = (int64_t)b * M + ee / N;
      const int n = (int)(ee % N) + 1;
      const float ca = coef[(row * (N + 1) + n) * 2], cc = coef[(row * (N + 1) + n) * 2 + 1];
      for (int c = lane; c < D; c += 64) dyr[c] += ca * x[row * D + c] - cc * yr[c];
    }
  }
}

}  // namespace

// ================================================================== C entries ===
extern "C" int lasr_w2v_conv0_fwd(const float* x, int B, int T_in, int C, int k, int s, const float* w,
                                  const float* bias, float* y, void* stream) {
  LASR_CHECK_ARG(B > 0 && C > 0 && k > 0 && s > 0 && T_in >= k, "lasr_w2v_conv0_fwd: bad shape");
  const int Tout = (T_in - k) / s + 1;
  conv0_fwd_kernel<<<grid1((int64_t)B * Tout * C), 256, 0, (hipStream_t)stream>>>(x, B, T_in, Tout, C, k, s, w, bias, y);
  return lasr_check_launch("w2v_conv0_fwd");
}

extern "C" int lasr_w2v_conv0_dw_parts(int B, int T_out) {
  const int64_t rows = (int64_t)B * T_out;
  const int64_t p = cdiv(rows, 512);
  return (int)(p < 1 ? 1 : p > 128 ? 128 : p);
}

extern "C" int lasr_w2v_conv0_dw(const float* x, const void* dy, int dy_dtype, int B, int T_in, int C, int k, int s,
                                 float* dw, float* ws, int64_t ws_floats, void* stream) {
  LASR_CHECK_ARG(B > 0 && C > 0 && k > 0 && k <= W2V_KMAX && s > 0 && T_in >= k && dt_ok(dy_dtype),
                 "lasr_w2v_conv0_dw: bad shape (k <= %d)", W2V_KMAX);
  const int Tout = (T_in - k) / s + 1;
  const int P = lasr_w2v_conv0_dw_parts(B, Tout);
  LASR_CHECK_ARG(ws && ws_floats >= (int64_t)P * C * k, "lasr_w2v_conv0_dw: workspace too small");
  const int64_t chunk = cdiv((int64_t)B * Tout, P);
  hipStream_t st = (hipStream_t)stream;
  conv0_dw_kernel<<<dim3((unsigned)cdiv(C, 64), (unsigned)P), dim3(64, 4), 0, st>>>(x, dy, dy_dtype, B, T_in, Tout, C, k,
                                                                                  s, chunk, ws);
  int rc = lasr_check_launch("w2v_conv0_dw");
  if (rc) return rc;
  return lasr_reduce_cols(ws, P, (int64_t)C * k, dw, nullptr, (int64_t)C * k, 1, st);
}

extern "C" int lasr_w2v_ln_act_fwd(const void* x, int x_dtype, int64_t rows, int C, const float* gamma,
                                   const float* beta, float eps, int act, void* y, int y_dtype, float* mean,
                                   float* rstd, void* stream) {
  LASR_CHECK_ARG(C > 0 && C <= 4096 && dt_ok(x_dtype) && dt_ok(y_dtype), "lasr_w2v_ln_act_fwd: C=%d unsupported", C);
  if (rows <= 0) return LASR_OK;
  ln_act_fwd_kernel<<<grid1(rows, 4), 256, 0, (hipStream_t)stream>>>(x, x_dtype, rows, C, gamma, beta, eps, act, y,
                                                                     y_dtype, mean, rstd);
  return lasr_check_launch("w2v_ln_act_fwd");
}

extern "C" int lasr_w2v_ln_act_bwd(const void* x, int x_dtype, const void* dy, int dy_dtype, int64_t rows, int C,
                                   const float* gamma, const float* beta, const float* mean, const float* rstd,
                                   int act, void* dx, int dx_dtype, float* dgamma, float* dbeta, float* ws,
                                   int64_t ws_floats, void* stream) {
  LASR_CHECK_ARG(C > 0 && C <= 1024 && dt_ok(x_dtype) && dt_ok(dy_dtype) && dt_ok(dx_dtype),
                 "lasr_w2v_ln_act_bwd: C=%d unsupported", C);
  if (rows <= 0) return LASR_OK;
  const int64_t nb = cdiv(rows, W2V_LN_ROWS);
  LASR_CHECK_ARG(ws && ws_floats >= nb * 2 * C, "lasr_w2v_ln_act_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  ln_act_bwd_kernel<<<(unsigned)nb, 256, (size_t)8 * C * sizeof(float), st>>>(x, x_dtype, dy, dy_dtype, rows, C, gamma,
                                                                             beta, mean, rstd, act, dx, dx_dtype, ws);
  int rc = lasr_check_launch("w2v_ln_act_bwd");
  if (rc) return rc;
  return lasr_reduce_cols(ws, (int)nb, 2 * (int64_t)C, dgamma, dbeta, C, 1, st);
}

extern "C" int lasr_w2v_col2im1d(const void* dcol, int dtype, int B, int T_in, int T_out, int C, int k, int s,
                                 float* dx, void* stream) {
  LASR_CHECK_ARG(B > 0 && C > 0 && k > 0 && s > 0 && T_out > 0 && (int64_t)s * (T_out - 1) + k <= T_in && dt_ok(dtype),
                 "lasr_w2v_col2im1d: bad shape");
  col2im1d_kernel<<<grid1((int64_t)B * T_in * C), 256, 0, (hipStream_t)stream>>>(dcol, dtype, B, T_in, T_out, C, k, s, dx);
  return lasr_check_launch("w2v_col2im1d");
}

extern "C" int lasr_w2v_group_pack(const float* src, int B, int T, int G, int cg, int front, int Tp, const void* yg,
                                   int yg_dtype, const float* bias, void* dst, int dst_dtype, void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && G > 0 && cg > 0 && front >= 0 && Tp >= front + T && dt_ok(dst_dtype) &&
                     (!yg || dt_ok(yg_dtype)),
                 "lasr_w2v_group_pack: bad shape");
  group_pack_kernel<<<grid1((int64_t)G * B * Tp * cg), 256, 0, (hipStream_t)stream>>>(src, B, T, G, cg, front, Tp, yg,
                                                                                     yg_dtype, bias, dst, dst_dtype);
  return lasr_check_launch("w2v_group_pack");
}

extern "C" int lasr_w2v_group_unpack(const void* yg, int yg_dtype, const float* bias, int act, const float* res, int B,
                                     int T, int G, int cg, float* out, void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && G > 0 && cg > 0 && dt_ok(yg_dtype), "lasr_w2v_group_unpack: bad shape");
  group_unpack_kernel<<<grid1((int64_t)B * T * G * cg), 256, 0, (hipStream_t)stream>>>(yg, yg_dtype, bias, act, res, B,
                                                                                      T, G, cg, out);
  return lasr_check_launch("w2v_group_unpack");
}

extern "C" int lasr_w2v_group_colsum(const void* x, int dtype, int G, int64_t rows, int cg, float* out, void* stream) {
  LASR_CHECK_ARG(G > 0 && rows > 0 && cg > 0 && dt_ok(dtype), "lasr_w2v_group_colsum: bad shape");
  group_colsum_kernel<<<(unsigned)(G * cg), 256, 0, (hipStream_t)stream>>>(x, dtype, rows, cg, out);
  return lasr_check_launch("w2v_group_colsum");
}

extern "C" int lasr_w2v_mask_fwd(float* x, const int32_t* midx, int B, int T, int M, int d, const float* mask_emb,
                                 void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && M >= 0 && d > 0, "lasr_w2v_mask_fwd: bad shape");
  if (M == 0) return LASR_OK;
  mask_fwd_kernel<<<grid1((int64_t)B * M * d), 256, 0, (hipStream_t)stream>>>(x, midx, B, T, M, d, mask_emb);
  return lasr_check_launch("w2v_mask_fwd");
}

extern "C" int lasr_w2v_mask_bwd(float* dx, const int32_t* midx, int B, int T, int M, int d, float* dmask_emb,
                                 void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && M >= 0 && d > 0, "lasr_w2v_mask_bwd: bad shape");
  if (M == 0) return LASR_OK;
  mask_bwd_kernel<<<grid1(d, 64), 64, 0, (hipStream_t)stream>>>(dx, midx, B, T, M, d, dmask_emb);
  return lasr_check_launch("w2v_mask_bwd");
}

extern "C" int lasr_w2v_gather_rows(const void* src, int src_dtype, int64_t stride_b, int64_t stride_t,
                                    const int32_t* midx, int B, int T, int M, int d, void* dst, int dst_dtype,
                                    void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && M > 0 && d > 0 && dt_ok(src_dtype) && dt_ok(dst_dtype),
                 "lasr_w2v_gather_rows: bad shape");
  gather_rows_kernel<<<grid1((int64_t)B * M * d), 256, 0, (hipStream_t)stream>>>(src, src_dtype, stride_b, stride_t, midx,
                                                                                B, T, M, d, dst, dst_dtype);
  return lasr_check_launch("w2v_gather_rows");
}

extern "C" int lasr_w2v_scatter_rows(const void* src, int src_dtype, const int32_t* midx, int B, int T, int M, int d,
                                     float* dst, int64_t stride_b, int64_t stride_t, int accumulate, void* stream) {
  LASR_CHECK_ARG(B > 0 && T > 0 && M > 0 && d > 0 && dt_ok(src_dtype), "lasr_w2v_scatter_rows: bad shape");
  scatter_rows_kernel<<<grid1((int64_t)B * M * d), 256, 0, (hipStream_t)stream>>>(src, src_dtype, midx, B, T, M, d, dst,
                                                                                 stride_b, stride_t, accumulate);
  return lasr_check_launch("w2v_scatter_rows");
}

extern "C" int lasr_w2v_gumbel_fwd(const void* logits, int dtype, const float* noise, uint64_t seed, float tau,
                                   int hard, int64_t R, int G, int V, const float* vars, int vd, void* out,
                                   int out_dtype, int32_t* codes, void* stream) {
  LASR_CHECK_ARG(R > 0 && G > 0 && V > 0 && vd > 0 && tau > 0.f && dt_ok(dtype) && dt_ok(out_dtype),
                 "lasr_w2v_gumbel_fwd: bad shape");
  const DropCfg dc = mkdrop(0.5f, seed);  // p only selects the step counter; the draw is gumbel_draw's
  gumbel_fwd_kernel<<<grid1(R * G, 4), 256, 0, (hipStream_t)stream>>>(logits, dtype, noise, dc, 1.f / tau, hard, R * G, G,
                                                                     V, vars, vd, out, out_dtype, codes);
  return lasr_check_launch("w2v_gumbel_fwd");
}

extern "C" int lasr_w2v_gumbel_bwd(const void* logits, int dtype, const float* noise, uint64_t seed, float tau,
                                   int hard, int64_t R, int G, int V, const float* vars, int vd, const void* dout,
                                   int dout_dtype, const int32_t* codes, void* dlogits, int dlogits_dtype,
                                   float* dvars, void* stream) {
  LASR_CHECK_ARG(R > 0 && G > 0 && V > 0 && V <= 8192 && vd > 0 && tau > 0.f && dt_ok(dtype) && dt_ok(dout_dtype) &&
                     dt_ok(dlogits_dtype),
                 "lasr_w2v_gumbel_bwd: bad shape (V <= 8192)");
  hipStream_t st = (hipStream_t)stream;
  if (hard) {  // eval: the one-hot comes from scatter_, no gradient reaches the logits
    int rc = lasr_fill(dlogits, dlogits_dtype, R * G * V, 0.f, stream);
    if (rc) return rc;
  } else {
    const DropCfg dc = mkdrop(0.5f, seed);
    gumbel_bwd_kernel<<<(unsigned)(R * G), 64, (size_t)V * sizeof(float), st>>>(logits, dtype, noise, dc, 1.f / tau, G, V,
                                                                              vars, vd, dout, dout_dtype, dlogits,
                                                                              dlogits_dtype);
    int rc = lasr_check_launch("w2v_gumbel_bwd");
    if (rc) return rc;
  }
  gumbel_dvars_kernel<<<(unsigned)(G * V), 64, 0, st>>>(codes, R, G, V, vd, dout, dout_dtype, dvars);
  return lasr_check_launch("w2v_gumbel_dvars");
}

extern "C" int lasr_w2v_contrast_fwd(const float* x, const float* y, const int32_t* neg, const int32_t* codes, int G,
                                     int B, int M, int N, int D, float logit_temp, float* logits, float* lse,
                                     float* row_loss, float* loss, void* stream) {
  LASR_CHECK_ARG(B > 0 && M > 0 && N >= 0 && N < 8192 && D > 0 && G > 0 && logit_temp > 0.f,
                 "lasr_w2v_contrast_fwd: bad shape");
  hipStream_t st = (hipStream_t)stream;
  contrast_fwd_kernel<<<(unsigned)(B * M), 64, (size_t)(N + 1) * sizeof(float), st>>>(
      x, y, neg, codes, G, B, M, N, D, 1.f / logit_temp, logits, lse, row_loss);
  int rc = lasr_check_launch("w2v_contrast_fwd");
  if (rc) return rc;
  mean_kernel<<<1, 256, 0, st>>>(row_loss, (int64_t)B * M, loss);
  return lasr_check_launch("w2v_contrast_mean");
}

extern "C" int lasr_w2v_contrast_bwd(const float* x, const float* y, const int32_t* neg, const int32_t* codes, int G,
                                     int B, int M, int N, int D, float logit_temp, const float* lse,
                                     const float* gout, float* dx, float* dy, float* ws, int64_t ws_floats,
                                     void* stream) {
  LASR_CHECK_ARG(B > 0 && M > 0 && N >= 0 && D > 0 && G > 0 && logit_temp > 0.f, "lasr_w2v_contrast_bwd: bad shape");
  LASR_CHECK_ARG(ws && ws_floats >= (int64_t)B * M * (N + 1) * 2, "lasr_w2v_contrast_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  contrast_bwd_x_kernel<<<(unsigned)(B * M), 64, 0, st>>>(x, y, neg, codes, G, B, M, N, D, 1.f / logit_temp, lse, gout,
                                                         dx, ws);
  int rc = lasr_check_launch("w2v_contrast_bwd_x");
  if (rc) return rc;
  contrast_bwd_y_kernel<<<(unsigned)(B * M), 64, 0, st>>>(x, y, neg, B, M, N, D, ws, dy);
  return lasr_check_launch("w2v_contrast_bwd_y");
}
