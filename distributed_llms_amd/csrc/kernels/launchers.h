// Host-side launcher declarations (C++ ABI, pointers as uintptr_t, stream as uintptr_t).
// Every launcher validates the shapes its grid assumes before launching.
#pragma once
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace dllm {

void rms_norm(uintptr_t y, uintptr_t x, uintptr_t residual, uintptr_t w, int rows, int hidden, float eps,
              uintptr_t stream);
void rms_norm_q8(uintptr_t y, uintptr_t x, uintptr_t residual, uintptr_t w, int rows, int hidden, float eps,
                 uintptr_t q8, uintptr_t qs, uintptr_t stream);
void splitk_add_rms_norm_q8(uintptr_t y, uintptr_t residual, uintptr_t ws, int S, int M, int N, uintptr_t w,
                            float eps, uintptr_t q8, uintptr_t qs, uintptr_t stream);
void embedding(uintptr_t out, uintptr_t ids, uintptr_t table, int tokens, int hidden, int vocab,
               uintptr_t stream);
void rope_cache_append(uintptr_t q_out, uintptr_t qkv, uintptr_t positions, uintptr_t cos_sin,
                       uintptr_t k_cache, uintptr_t v_cache, uintptr_t slots, int tokens, int hq, int hkv,
                       int d, int bs, int v_groups, uintptr_t stream);
// qkv_prep.hip: Qwen2 qkv bias (bias [(Hq + 2 Hkv) D] or 0) and Qwen3 per-head RMSNorm over D on the q / k heads
// (q_w / k_w [D] or 0), in place on the dense qkv [T, (Hq + 2 Hkv) D]; D is 64 or 128
void qkv_prep(uintptr_t qkv, uintptr_t bias, uintptr_t q_w, uintptr_t k_w, int tokens, int hq, int hkv, int d,
              float eps, uintptr_t stream);
void silu_mul(uintptr_t out, uintptr_t gu, int tokens, int inter, uintptr_t stream);
void add_inplace(uintptr_t a, uintptr_t b, long n, uintptr_t stream);
void argmax(uintptr_t out, uintptr_t logits, int rows, int vocab, long row_stride, uintptr_t stream);
// sampler.hip: params [rows, 3] i32 (temperature * 1e4, top_k, top_p * 1e4), seeds [rows] u64, pos [rows] i32,
// uniforms [rows] f32 or 0 (test hook: replaces the Philox draw); all on the device
void sample_rows(uintptr_t out_ids, uintptr_t logits, int rows, int vocab, long row_stride, uintptr_t params,
                 uintptr_t seeds, uintptr_t pos, uintptr_t uniforms, uintptr_t stream);
// sampler.hip: log-probabilities of the model's distribution.  ids [rows] i32 (the chosen token), want [rows] i32
// (-1: skip the row, else how many top entries, at most n_max); chosen [rows] f32, top_ids / top_lp [rows, n_max]
constexpr int kMaxLogprobs = 20;
void token_logprobs(uintptr_t chosen, uintptr_t top_ids, uintptr_t top_lp, uintptr_t logits, int rows, int vocab,
                    long row_stride, uintptr_t ids, uintptr_t want, int n_max, uintptr_t stream);
// logit_processors.hip: penalties, logit_bias and the min_tokens EOS ban on the bf16 logits, in place.  state
// [state_rows, pitch] u32 (one row per asking request), procs [rows, kProcWords] i32 (the layout is in the file's
// head), bias_n [state_rows] i32, bias_ids / bias_vals [state_rows, bias_pitch]; step_bias_* the lists a step installs
// (cu [rows + 1]); all on the device
constexpr int kProcWords = 8;
void apply_logit_processors(uintptr_t logits, int rows, int vocab, long row_stride, uintptr_t state, int pitch,
                            int state_rows, uintptr_t procs, uintptr_t seq_lens, int eos_id, uintptr_t bias_n,
                            uintptr_t bias_ids, uintptr_t bias_vals, int bias_pitch, uintptr_t stream);
void logit_state_update(uintptr_t state, int pitch, int state_rows, int vocab, uintptr_t ids, uintptr_t cu_seqlens,
                        uintptr_t procs, int rows, uintptr_t bias_n, uintptr_t bias_ids, uintptr_t bias_vals,
                        int bias_pitch, uintptr_t step_bias_cu, uintptr_t step_bias_ids, uintptr_t step_bias_vals,
                        uintptr_t stream);
void logit_state_count(uintptr_t state, int pitch, int state_rows, int vocab, uintptr_t ids, uintptr_t procs, int rows,
                       uintptr_t stream);

// lora.hip: per-row adapters after a projection.  tile_slot [nt] / tile_rows [nt * 16] i32: the step's row plan
// (-1: unused tile / padding); A [slots, R, K] bf16 (R = slices x rp), B [slots, N, rp] bf16, scale [slots] f32;
// ws: f32 [lora_ksplit(K), nt * 16, R]; off1 / off2: first column of slice 1 / 2 (N when there is none)
int lora_ksplit(int K);
void lora_shrink(uintptr_t ws, long ws_floats, uintptr_t x, uintptr_t A, uintptr_t tile_slot, uintptr_t tile_rows,
                 int T, int K, int R, int nslots, int nt, uintptr_t stream);
void lora_expand(uintptr_t y, long ldy, uintptr_t ws, long ws_floats, uintptr_t B, uintptr_t scale,
                 uintptr_t tile_slot, uintptr_t tile_rows, int T, int N, int K, int R, int rp, int off1, int off2,
                 int nslots, int nt, uintptr_t stream);

void splitk_add_rms_norm(uintptr_t y, uintptr_t residual, uintptr_t ws, int S, int M, int N, uintptr_t w, float eps,
                         uintptr_t stream);
void splitk_reduce(uintptr_t out, uintptr_t ws, uintptr_t bias, int S, int M, int N, uintptr_t stream);
void splitk_reduce_ex(uintptr_t out, uintptr_t ws, uintptr_t bias, int S, int M, int N, int swiglu,
                      uintptr_t stream);
int gemm_wide(uintptr_t c, uintptr_t a, uintptr_t b, uintptr_t ws, long ws_floats, int M, int N, int K, int splits,
              int mode, int variant, uintptr_t stream);
int gemm_wide_fp8(uintptr_t c, uintptr_t a, uintptr_t a_scale, uintptr_t b, uintptr_t b_scale, uintptr_t ws,
                  long ws_floats, int M, int N, int K, int splits, int mode, int variant, uintptr_t stream);
void quant_fp8_rows(uintptr_t q, uintptr_t scale, uintptr_t x, int M, int K, uintptr_t stream);
int gemm_pp(uintptr_t c, uintptr_t a, uintptr_t b, uintptr_t ws, long ws_floats, int M, int N, int K, int splits,
            int mode, int variant, uintptr_t stream);
void gemm_pp_moe(uintptr_t y, uintptr_t x, uintptr_t gather, uintptr_t w, uintptr_t counts, uintptr_t offsets, int E,
                 int N, int K, int xrows, int slots, int mode, uintptr_t stream);
void gemm_pf(uintptr_t c, uintptr_t a, uintptr_t b, int M, int N, int K, int mode, int variant, uintptr_t stream);
int gemm_sq(uintptr_t c, uintptr_t a, uintptr_t b, uintptr_t ws, long ws_floats, int M, int N, int K, int splits,
            int mode, int variant, uintptr_t stream);

void moe_route(uintptr_t logits, int T, int E, int k, uintptr_t topk_w, uintptr_t topk_ids, uintptr_t counts,
               uintptr_t offsets, uintptr_t sorted_tok, uintptr_t inv, uintptr_t stream);
void moe_grouped_gemm(uintptr_t y, uintptr_t x, uintptr_t gather, uintptr_t w, uintptr_t counts, uintptr_t offsets,
                      int E, int N, int K, int mode, int rows_hint, int variant, uintptr_t stream);
void moe_router_route(uintptr_t x, uintptr_t w, int T, int H, int E, int k, uintptr_t topk_w, uintptr_t topk_ids,
                      uintptr_t counts, uintptr_t offsets, uintptr_t sorted_tok, uintptr_t inv, uintptr_t stream);
void moe_wide_gemm(uintptr_t y, uintptr_t x, uintptr_t gather, uintptr_t w, uintptr_t counts, uintptr_t offsets,
                   int E, int N, int K, int mode, uintptr_t stream);
void moe_wide_gemm_fp8(uintptr_t y, uintptr_t x, uintptr_t gather, uintptr_t w, uintptr_t counts, uintptr_t offsets,
                       int E, int N, int K, int mode, uintptr_t sa, uintptr_t wscale, uintptr_t stream);
void moe_combine(uintptr_t out, uintptr_t ysorted, uintptr_t topk_w, uintptr_t inv, int T, int H, int k,
                 uintptr_t stream);

void paged_attention_decode(uintptr_t out, uintptr_t q, uintptr_t k_cache, uintptr_t v_cache,
                            uintptr_t block_tables, uintptr_t seq_lens, uintptr_t part_o, uintptr_t part_ml,
                            int batch, int hq, int hkv, int d, int block_size, int max_blocks, int num_splits,
                            int split_len, float scale, uintptr_t stream);
void paged_attention_decode_rope(uintptr_t out, uintptr_t qkv, uintptr_t positions, uintptr_t cos_sin, uintptr_t slots,
                                 uintptr_t k_cache, uintptr_t v_cache, uintptr_t block_tables, uintptr_t seq_lens,
                                 uintptr_t part_o, uintptr_t part_ml, int batch, int hq, int hkv, int d,
                                 int block_size, int max_blocks, int num_splits, int split_len, float scale,
                                 uintptr_t qkv_part, int qkv_nparts, long qkv_slab, uintptr_t stream);
void paged_attention_prefill(uintptr_t out, uintptr_t q, uintptr_t k_cache, uintptr_t v_cache,
                             uintptr_t block_tables, uintptr_t cu_seqlens_q, uintptr_t seq_lens, int batch,
                             int hq, int hkv, int d, int block_size, int max_blocks, int max_q_len, float scale,
                             int version, uintptr_t positions, uintptr_t cos_sin, int q_stride, uintptr_t stream);
// prefill version 5 (split context): partials [T, hq, nsplit, D] / [T, hq, nsplit, 2] floats + the split reduce
void paged_attention_prefill_split(uintptr_t out, uintptr_t q, uintptr_t k_cache, uintptr_t v_cache,
                                   uintptr_t block_tables, uintptr_t cu_seqlens_q, uintptr_t seq_lens,
                                   uintptr_t part_o, uintptr_t part_ml, int batch, int total_tokens, int hq, int hkv,
                                   int d, int block_size, int max_blocks, int max_q_len, int max_ctx, int nsplit,
                                   int split_chunks, float scale, uintptr_t stream);

long p2p_inbox_bytes(long chunk, int nslots);
void p2p_standin(uintptr_t src, uintptr_t s_inbox, long s_bytes, uint64_t s_seq0, uintptr_t dst, uintptr_t r_inbox,
                 long r_bytes, uint64_t r_seq0, long chunk, int nslots, int channels, uintptr_t abort_word,
                 double timeout_s, uintptr_t err, int lds_bytes, uintptr_t stream);
uintptr_t p2p_host_words(int n);
void p2p_host_words_free(uintptr_t p);

}  // namespace dllm
