/*
 * asm_hip_debug.h -- TEST-ONLY entry points of libasm_hip.so.  Not part of the drop-in boundary (include/asm_hip.h):
 * nothing in the product package calls them; tests/ uses them to cross-check the MFMA kernels at sizes the CPU
 * oracle cannot reach and to assert which kernel plan a shape gets.
 */
#ifndef ASM_HIP_DEBUG_H_
#define ASM_HIP_DEBUG_H_

#include "asm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Direct convolutions (one thread per output element, fp32 accumulate, same descriptor / layouts as the MFMA
 * kernels): the definition of conv2d_fixed_padding (nets/model_helper.py:67-78) and of its two gradients written
 * as plain loops. */
int asm_conv2d_fprop_naive(const asm_conv_desc* d, const void* x, const void* w, void* y, void* stream);
int asm_conv2d_dgrad_naive(const asm_conv_desc* d, const void* dy, const void* w_krsc, void* dx, void* stream);
int asm_conv2d_wgrad_naive(const asm_conv_desc* d, const void* x, const void* dy, float* dw, void* stream);

/* Each lane l of one wave reads ds_read_b64_tr_b16 at LDS element 4*l of lds[i] = i; out[l*4+j]. */
int asm_debug_tr_probe(void* out256_i16, void* stream);

/* The weight-gradient plan asm_conv2d_wgrad would use for d (with the current ASM_WGRAD_* knobs):
 * plan = {dy-tile rows (32/64/128/256), column-tile width (128/256), tiles_n, tiles_c, pixel splits, pixels per split}.
 * Column-tile width -1: the resident-halo form, {K, -1, 1, 1, workgroups per K slice (= slabs), pixels per workgroup};
 * -2: the [N,1,1,C] layer on dense_small_wgrad_kernel, {K, -2, ceil(K/32), ceil(C/32), 1, N}. */
int asm_conv2d_wgrad_plan(const asm_conv_desc* d, int32_t plan[6]);

/* Kernel family of the calling thread's last asm_conv2d_fprop* / asm_conv2d_dgrad* launch: 0 igemm_kernel (general fallback),
 * 1 igemm1_kernel (1x1 ring GEMM), 2 igemm2_kernel, 3 igemm3_kernel (rows resident across the taps), 4 conv_halo_kernel,
 * 5 dgrad_s2_kernel, 6 dense_small_kernel (a [N,1,1,C] layer), 8 igemm8_kernel (wave-staggered multi-phase loop); -1 before the first call. */
int asm_debug_last_conv_kernel(void);

/* asm_retrieval_topk_wide with the same arguments and result, which also ADDS to three device counters (uint64, zeroed by the
 * caller): {candidates appended to the (query, run) buffers, compactions during the index walk, compactions at the end of a
 * run}.  tools/retrieval_bench.py --counters reports them per query. */
int asm_debug_retrieval_topk_wide_counted(const void* queries, int ldq, const void* index, int ldi, const float* sq_queries,
                                          const float* sq_index, int Q, int N, int D, int similarity, int K, int index_base,
                                          float* top_val, int32_t* top_idx, void* workspace, size_t workspace_bytes,
                                          void* stream, unsigned long long* counters3);

/* The plan of the list selection (wide = 0: asm_retrieval_topk) or of the wide one (wide != 0: asm_retrieval_topk_wide) for
 * Q queries, N index rows and K results, read from the RetrievalPlan that the one launcher of both entry points acts on:
 * plan = {S index splits (runs), 128-row tiles per split, tiles in all, capacity B of a (query, run) candidate buffer (0 for
 * the list selection)}.  S == 1 on the list path: the kernel writes the result itself, no merge launch.  The last split holds
 * tiles - (S - 1) * tiles_per_split tiles.  Host only: nothing is launched.  A non-positive size or a null plan -> ASM_EINVAL,
 * K above the selection's cap -> ASM_ENOTSUP. */
int asm_debug_retrieval_plan(int Q, int N, int K, int wide, int32_t plan[4]);


#ifdef __cplusplus
}
#endif
#endif /* ASM_HIP_DEBUG_H_ */
