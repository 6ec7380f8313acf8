// Phased main loop for the long-K, N = d GEMMs (FFN fc2 forward, FFN fc1 input gradient, the
// subsampling output projection): one 128 x 64 workgroup per CU, the LDS-DMA ring kept in
// flight across raw barriers, and every fragment read and DMA issue placed between the MFMAs
// of the sub-tile before it.  Same LDS images, fragment reads, MFMA operand order and epilogue
// as gemm_bf16_glds_kernel (gemm_kernel.h), and every accumulator takes its 32-deep k chunks in
// ascending order: the outputs are the bits of that kernel.
//
// Geometry: 4 waves as 2 (M) x 2 (N), each owning 64 x 32 (FM 4 x FN 2 accumulators of
// v_mfma_f32_16x16x32_bf16).  A is K-contiguous; B is K-contiguous (ds_read_b128 fragments)
// or N-contiguous (ds_read_b64_tr_b16 fragments).  A ring stage is 64 deep: two 32-deep
// sub-tiles (A image 128 x 32 + B image 64 x 32 = 12 KB each), GL = 6 global_load_lds_dwordx4
// per thread.  The ring holds S stages and the DMA runs D = S - 1 stages ahead of the MFMAs.
//
// With one wave per SIMD nothing hides a wave's own instruction issue, so the loop is written
// as MFMAs with the other work in their shadow: after each MFMA (16 cycles of the matrix pipe)
// come at most three other instructions.  Iteration kt (one stage, one barrier, 16 MFMAs per
// wave); f0 / f1 = the fragment register sets of the stage's two sub-tiles:
//   top      s_waitcnt vmcnt(GL * (D - 3))      this wave's part of stage kt+2 has landed
//            s_barrier                           (raw: the ring stays in flight)
//            s_waitcnt lgkmcnt(0)                f0 = (kt, 0), read in iteration kt-1
//   group A  8 MFMAs on f0; between them: ds_read (kt, 1) -> f1; then LDS-DMA (kt+D, 0)
//            s_waitcnt lgkmcnt(0)                f1
//   group B  8 MFMAs on f1; between them: ds_read (kt+1, 0) -> f0; then LDS-DMA (kt+D, 1)
// s_setprio 1 / 0 bracket each group.
//
// Why the counts are right (placement by counting, not by clean runs):
//  RAW, DMA -> ds_read.  Stage kt+1 is first read in group B of iteration kt.  DMAs retire in
//    issue order per wave.  At the top of iteration kt the wave has issued the stages up to
//    min(kt-1+D, nst-1); those after kt+2 are at most D - 3 stages of GL instructions, so the
//    counted vmcnt leaves nothing of stage kt+2 or older outstanding in this wave, and the
//    barrier extends that to the four waves (each wrote a quarter of every image).  Stage kt+1
//    was retired the same way at the top of iteration kt-1 (stages 0 and 1: in the prologue),
//    so it is read one whole iteration after the wait and barrier that retired it, never in
//    the iteration of its own wait.
//  WAR, ds_read -> DMA.  The DMA of iteration kt overwrites the slot of stage kt+D-S = kt-1.
//    Its last reads are those of (kt-1, 1), issued in group A of iteration kt-1 and complete at
//    that iteration's second lgkmcnt(0), and those of (kt-1, 0), complete at its first; every
//    wave passes both before it reaches the barrier of iteration kt, and the DMA is issued
//    after that barrier.
//  Fragment registers: f1 is reloaded in group A after the MFMAs of the previous group B were
//    issued (in-order issue), f0 likewise in group B.
//  The epilogue reuses the ring's LDS after the last lgkmcnt(0), vmcnt(0) and a barrier.
#include "gemm_phase.h"

#include <atomic>
#include <type_traits>

namespace {

constexpr int PH_BM = 128, PH_BN = 64;

// vmcnt(GL * n), n = stages left in flight (0 .. NMAX): a uniform branch to the immediate
template <int GL, int NMAX>
LASR_DEV void wait_stages(int n) {
  if constexpr (NMAX > 0) {
    if (n >= NMAX) { wait_vmcnt<GL * NMAX>(); return; }
    wait_stages<GL, NMAX - 1>(n);
  } else {
    wait_vmcnt<0>();
  }
}

LASR_DEV v4i ds_b128_at(uint32_t addr, int off) {
  v4i r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(off));
  return r;
}
LASR_DEV v2i ds_tr_at(uint32_t addr) {
  v2i r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}

// One fragment register set: the A fragments of the wave's 4 row groups and the B fragments of
// its 2 column groups for one 32-deep sub-tile.
template <bool BKC>
struct PhaseFrags {
  v4i a[4];
  v4i bk[BKC ? 2 : 1];
  v2i bt[BKC ? 1 : 4];
};

// s_waitcnt lgkmcnt(0) that the set's MFMAs depend on (in/out operands)
template <bool BKC>
LASR_DEV void frags_wait(PhaseFrags<BKC>& f) {
  if constexpr (BKC)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.bk[0]), "+v"(f.bk[1]));
  else
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.bt[0]), "+v"(f.bt[1]),
                   "+v"(f.bt[2]), "+v"(f.bt[3]));
}

LASR_DEV void pin() { __builtin_amdgcn_sched_barrier(0); }

template <bool BKC, typename TC, int EPI, int S>
__global__ __launch_bounds__(256, 1) void gemm_phase_kernel(GemmP p) {
  constexpr int BM = PH_BM, BN = PH_BN, BK = 32, NT = 256;
  constexpr int WM = 64, WN = 32, FM = 4, FN = 2;
  constexpr int TILE = (BM + BN) * BK;  // elements per sub-tile image
  constexpr int STAGE = 2 * TILE, D = S - 1, GL = 2 * (BM + BN) * 4 / NT;
  constexpr int MAIN_BYTES = S * STAGE * 2, EPI_BYTES = WM * (BN + 4) * 4;
  static_assert(S >= 5, "vmcnt(GL * (D - 3)) must leave a stage in flight");
  static_assert(MAIN_BYTES >= EPI_BYTES && MAIN_BYTES <= 160 * 1024, "ring size");
  static_assert(GL * (D - 3) < 64, "vmcnt range");
  // all LDS of the kernel (ring and epilogue staging) is this one array
  __shared__ __attribute__((aligned(16))) char smem_epi[MAIN_BYTES];
  bf16_t* smem = reinterpret_cast<bf16_t*>(smem_epi);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  const int nx = gridDim.x, ny = gridDim.y;
  const int wg = xcd_remap(blockIdx.y * nx + blockIdx.x, nx * ny);
  const int tx = wg % nx, ty = wg / nx;
  const int m0 = ty * BM, n0 = tx * BN;
  const int nst = p.K / (2 * BK);  // host-checked: K % 64 == 0, K >= 64

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- LDS-DMA sources: the 16-B positions of glds_tile (tile.h; the swizzles on the source
  // side), as one loop-invariant 32-bit byte offset per position beside a uniform base that
  // advances with k (host-checked: the operands span < 4 GB).  Rows past M / N read clamped.
  uint32_t va[2], vb;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int P = i * NT + tid, r = P >> 2, c = (P & 3) ^ swz(r);
    va[i] = 2u * ((uint32_t)min(m0 + r, p.M - 1) * (uint32_t)p.lda_m + (uint32_t)c * 8u);
  }
  if constexpr (BKC) {
    const int r = tid >> 2, c = (tid & 3) ^ swz(r);
    vb = 2u * ((uint32_t)min(n0 + r, p.N - 1) * (uint32_t)p.ldb_n + (uint32_t)c * 8u);
  } else {
    constexpr int CPR = BN / 8;
    const int k = tid / CPR, ps = tid % CPR;
    const int ls = ((((ps >> 1) ^ htr<BN>(k))) << 1) | (ps & 1);
    const int gc = min(n0 + ls * 8, ((p.N + 7) & ~7) - 8);
    vb = 2u * ((uint32_t)k * (uint32_t)p.ldb_k + (uint32_t)gc);
  }
  // the next sub-tile to issue (sub-tiles are issued in k order: a running uniform base each)
  const char* adma = (const char*)p.A;
  const char* bdma = (const char*)p.B;
  const int64_t bstep = BKC ? 2 * BK : 2 * BK * p.ldb_k;  // bytes of B per sub-tile of k
  const int wid_s = __builtin_amdgcn_readfirstlane(wid);
  auto issue_sub = [&](int slot, int u) {  // into sub-tile image u of ring slot `slot`
    if (LASR_EXP & 4) return;
    bf16_t* dst = smem + slot * STAGE + u * TILE + wid_s * 512;
    __builtin_amdgcn_global_load_lds((gptr_t)(adma + va[0]), (lptr_t)dst, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(adma + va[1]), (lptr_t)(dst + NT * 8), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(bdma + vb), (lptr_t)(dst + BM * BK), 16, 0, 0);
  };
  auto advance = [&]() {
    adma += 2 * BK;
    bdma += bstep;
  };

  // ---- fragment reads: per-thread image offsets (bytes); rows 16 apart keep their chunk
  // swizzle (swz reads row bits 2-3), so fragment i of a K-contiguous image is 1 KB * i on
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
  const uint32_t a_off = lds0 + 2u * (uint32_t)lds_off(wr * WM + (lane & 15), lane >> 4);
  [[maybe_unused]] const uint32_t bk_off =
      lds0 + 2u * (uint32_t)(BM * BK + lds_off(wc * WN + (lane & 15), lane >> 4));
  [[maybe_unused]] uint32_t bt_off[FN][2];
  if constexpr (!BKC)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      frag_tr_offsets<BN>(wc * WN + j * 16, lane, bt_off[j]);
      bt_off[j][0] += lds0 + 2u * BM * BK;
      bt_off[j][1] += lds0 + 2u * BM * BK;
    }
  // part n (0..2) of the reads of the sub-tile at byte offset `sub` of the ring
  auto read_part = [&](PhaseFrags<BKC>& f, uint32_t sub, int n) {
    if (n == 0) {
      f.a[0] = ds_b128_at(a_off + sub, 0);
      f.a[1] = ds_b128_at(a_off + sub, 1024);
    } else if (n == 1) {
      f.a[2] = ds_b128_at(a_off + sub, 2048);
      f.a[3] = ds_b128_at(a_off + sub, 3072);
    } else if constexpr (BKC) {
      f.bk[0] = ds_b128_at(bk_off + sub, 0);
      f.bk[1] = ds_b128_at(bk_off + sub, 1024);
    } else {
      f.bt[0] = ds_tr_at(bt_off[0][0] + sub);
      f.bt[1] = ds_tr_at(bt_off[0][1] + sub);
      f.bt[2] = ds_tr_at(bt_off[1][0] + sub);
      f.bt[3] = ds_tr_at(bt_off[1][1] + sub);
    }
  };
  // MFMA n (0..7) of a sub-tile: acc[n / 2][n % 2].  Swapped operands, as gemm_glds_tile:
  // acc[i][j] accumulates the C^T fragment.
  auto mfma = [&](const PhaseFrags<BKC>& f, int n) {
    const int i = n >> 1, j = n & 1;
    const bf16x8 af = __builtin_bit_cast(bf16x8, f.a[i]);
    bf16x8 bfr;
    if constexpr (BKC) bfr = __builtin_bit_cast(bf16x8, f.bk[j]);
    else bfr = frag_from_raw(f.bt + 2 * j);
    if (LASR_EXP & 1) {
      acc[i][j][0] += (float)af[0] + (float)bfr[0];
      return;
    }
    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr, af, acc[i][j], 0, 0, 0);
  };
  // 8 MFMAs on `cur` with the reads of the next sub-tile (at `nsub`) into `nxt` after MFMAs 0-2
  // and the DMA of the next sub-tile in k order (when `dma`) behind the last (the uniform branch
  // around it stays out of the MFMA sequence: inside, hipcc moved an accumulator through VGPRs)
  auto group = [&](const PhaseFrags<BKC>& cur, PhaseFrags<BKC>& nxt, uint32_t nsub, bool dma, int slot, int u) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      mfma(cur, n);
      pin();
      if (n < 3) read_part(nxt, nsub, n);
      pin();
    }
    if (dma) issue_sub(slot, u);
    advance();
    pin();
    __builtin_amdgcn_s_setprio(0);
  };

  PhaseFrags<BKC> f0, f1;
#pragma unroll
  for (int t = 0; t < D; ++t)
    if (t < nst) {
      issue_sub(t, 0);
      advance();
      issue_sub(t, 1);
      advance();
    }
  wait_stages<GL, D - 2>(min(D, nst) - 2);  // stages 0 and 1
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int n = 0; n < 3; ++n) read_part(f0, 0u, n);
  int slot = 0;  // kt % S
  for (int kt = 0; kt < nst; ++kt) {
    const bool dma = kt + D < nst;
    // stage kt+2 (the counts: header); the ring running dry takes the branch to a smaller count
    if (kt + D <= nst) wait_vmcnt<GL * (D - 3)>();
    else wait_stages<GL, D - 3>(nst - 1 - (kt + 2));
    __builtin_amdgcn_s_barrier();
    const int nslot = slot + 1 == S ? 0 : slot + 1;  // (kt+1) % S
    const int dslot = slot == 0 ? S - 1 : slot - 1;  // (kt+D) % S
    const uint32_t sub0 = (uint32_t)slot * (STAGE * 2);
    frags_wait<BKC>(f0);
    group(f0, f1, sub0 + TILE * 2, dma, dslot, 0);
    frags_wait<BKC>(f1);
    // (the last iteration reads slot nst % S, which no DMA writes any more, into the idle set)
    group(f1, f0, (uint32_t)nslot * (STAGE * 2), dma, dslot, 1);
    slot = nslot;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the idle set's reads
  // the last iteration waited vmcnt(0) in every wave
  __syncthreads();
  // host-checked (gemm_phased_launch): the epilogue's fast path, so its generic one is not built
  __builtin_assume(p.split_k <= 1 && p.epi_mode < 2);
  gemm_epilogue<BM, BN, TC, true, G_LIN, 4, EPI>(p, acc, smem_epi, m0, n0, 0, 0, 0, 0);
}

constexpr int PH_S = 6;  // ring stages (64 deep, 24 KB): 144 KB of LDS, 5 stages ahead

template <bool BKC>
void launch_phase(const GemmP& p, int epi, dim3 grid, hipStream_t st) {
  if (epi == EPI_RES_DROP) gemm_phase_kernel<BKC, float, EPI_RES_DROP, PH_S><<<grid, 256, 0, st>>>(p);
  else gemm_phase_kernel<BKC, bf16_t, EPI_PLAIN, PH_S><<<grid, 256, 0, st>>>(p);
}

std::atomic<long long> phased_launches{0};
// 1 = route by the predicates below (default), 0 = never, 2 = whatever the sizes
// (lasr_gemm_phased: A/B tools and the tests flip it inside one process)
std::atomic<int> phased_mode{1};

// CUs of the device that is current at the first call, kept for the process (one device per
// process, as everywhere in this library)
int cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
  }();
  return n;
}

}  // namespace

bool gemm_phased_launch(const lasr_gemm_args* a, const GemmP& p, bool glds, hipStream_t st) {
  const int mode = phased_mode.load(std::memory_order_relaxed);
  if (!mode) return false;
  // operands: bf16, LDS-DMA eligible (16-B aligned rows), A K-contiguous, one problem
  if (!glds || a->lda_k != 1 || p.batch != 1 || p.split_k > 1 || a->rowsum || a->zout) return false;
  if (a->K < 64 || a->K % 64 != 0) return false;
  const int e = epi_code(p);
  const bool res_drop = e == EPI_RES_DROP && a->c_dtype == LASR_F32;
  const bool plain = e == EPI_PLAIN && a->c_dtype == LASR_BF16;
  if (!res_drop && !plain) return false;
  // the kernel's 32-bit DMA source offsets
  const bool bkc = a->ldb_k == 1;
  const int64_t a_bytes = 2 * (int64_t)a->M * a->lda_m, b_bytes = 2 * (bkc ? (int64_t)a->N * a->ldb_n : 32 * a->ldb_k);
  if (a_bytes >= (1ll << 32) || b_bytes >= (1ll << 32)) return false;
  const int64_t tiles = cdiv(a->M, PH_BM) * cdiv(a->N, PH_BN);
  if (mode != 2) {
    // long K, and about one workgroup per CU (3/4 to 1 x the CU count)
    const int cus = cu_count();
    if (a->K < 1024 || cus <= 0 || tiles > cus || tiles * 4 < (int64_t)cus * 3) return false;
  }
  if (cdiv(a->M, PH_BM) > 65535) return false;
  dim3 grid((unsigned)cdiv(a->N, PH_BN), (unsigned)cdiv(a->M, PH_BM), 1);
  if (bkc) launch_phase<true>(p, e, grid, st);
  else launch_phase<false>(p, e, grid, st);
  return true;
}

void gemm_phased_count() { phased_launches.fetch_add(1, std::memory_order_relaxed); }

extern "C" int lasr_gemm_phased(int mode) {
  LASR_CHECK_ARG(mode >= 0 && mode <= 2, "lasr_gemm_phased: mode 0 (never), 1 (by size) or 2 (force)");
  phased_mode.store(mode, std::memory_order_relaxed);
  return LASR_OK;
}

extern "C" long long lasr_gemm_phased_launches(void) { return phased_launches.load(std::memory_order_relaxed); }
