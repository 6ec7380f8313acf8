// The phased 128 x 64 GEMM kernel (gemm_phase.hip) as lasr_gemm's launcher sees it.
#pragma once
#include "gemm_kernel.h"

// Launches call `a` (already lowered to `p`; `glds` = LDS-DMA eligible operands) on the phased
// kernel and returns true when the call is one of its shapes: bf16, A K-contiguous, K % 64 == 0
// and K >= 1024, no split / rowsum / zout, epilogue EPI_RES_DROP (fp32) or EPI_PLAIN (bf16),
// and 128 x 64 tiles numbering 3/4 to 1 x the CU count.  false: nothing was launched and the
// call keeps its planned instance.  lasr_gemm_phased(0 / 2): never / ignore the size predicates.
bool gemm_phased_launch(const lasr_gemm_args* a, const GemmP& p, bool glds, hipStream_t st);
// One more routed call for lasr_gemm_phased_launches(); the caller counts after its launch check.
void gemm_phased_count();
