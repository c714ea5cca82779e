/*
 * recsys_amd.h -- C ABI of librecsys_amd.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the two hot paths of NVIDIA/recsys-examples:
 *   A. DynamicEmb lookup  -- replaces the pybind11 module `dynamicemb_extensions`
 *      (corelib/dynamicemb/src/module_bind.cu:33-44); every entry point below cites the
 *      reference function it stands in for.
 *   B. HSTU jagged attention -- replaces `hstu_attn_2_cuda.varlen_fwd / varlen_bwd`
 *      (corelib/hstu/csrc/hstu_attn/hstu_api.cpp:335-725) / `torch.ops.fbgemm.hstu_varlen_{fwd,bwd}_*`.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (unless a parameter says "host"), sizes, a hipStream_t.
 *     No torch types.  The caller owns every buffer; nothing is allocated or freed here.
 *   - every function returns 0 on success, MI355_EINVAL (-1) for a rejected argument,
 *     MI355_ELAUNCH (-2) for a HIP launch error; mi355_last_error() holds the message
 *     (thread local).  Per-key failure is DATA (index -1, InsertResult), never an error code,
 *     as in the reference (src/check.h:40-60; kernels.cuh).
 *   - everything is asynchronous on `stream`; no entry point synchronises the host.
 *   - `n_dev` / `nu_dev` (nullable): the element count may live on the device; kernels are
 *     launched for the upper bound `n` and use min(n, *n_dev).  This removes the host syncs
 *     the reference API bakes in (h_num_missing, num_evicted.item(), ...).
 *   - keys are 64-bit (int64 or uint64 bit patterns), indices/offsets int64, as in the reference.
 *   - dtype codes: 0 = float32, 1 = bfloat16, 2 = float16.
 *   - scratch comes from the caller: mi355_*_workspace_bytes() gives the size.
 *
 * Reference paths are relative to /root/reference/corelib/dynamicemb/ unless noted.
 */
#ifndef RECSYS_AMD_H_
#define RECSYS_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

#define MI355_OK 0
#define MI355_EINVAL (-1)
#define MI355_ELAUNCH (-2)

/* ScorePolicy: src/table_operation/score.cuh:30-43 (pybind enum table.cu:186-192) */
enum { MI355_POLICY_CONST = 0, MI355_POLICY_ASSIGN = 1, MI355_POLICY_ACCUMULATE = 2,
       MI355_POLICY_GLOBAL_TIMER = 3, MI355_POLICY_LRU_LFU = 4 };
/* InsertResult: src/table_operation/types.cuh:52-61 */
enum { MI355_RES_INSERT = 0, MI355_RES_RECLAIM = 1, MI355_RES_ASSIGN = 2, MI355_RES_EVICT = 3,
       MI355_RES_DUPLICATED = 4, MI355_RES_BUSY = 5, MI355_RES_ILLEGAL = 6, MI355_RES_INIT = 7 };

const char* mi355_last_error(void);
int mi355_abi_version(void);

/* ------------------------------------------------------------------ scored hash table ---- */

/* LinearBucketTable._init_table, scored_hashtable.py:476-495 (keys = Empty, scores = 0,
 * digests = empty digest).  storage: num_buckets * C * (9 + 8*num_scores) bytes. */
int mi355_table_init(void* storage, int64_t num_buckets, int64_t bucket_capacity, int64_t num_scores,
                     hipStream_t stream);

/* table_lookup, src/table_operation/lookup.cu:151-191 + table_lookup_kernel kernels.cuh:81-187.
 * founds: uint8 (bool), indices: table-relative slot or -1, score_out as the reference.
 * timer_override != 0 replaces the device clock for GLOBAL_TIMER / LRU_LFU (test hook). */
int mi355_table_lookup(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                       int64_t num_scores, int64_t n, const int64_t* n_dev, const void* keys,
                       const int64_t* table_ids, const void* score_in, int policy, uint64_t timer_override,
                       int64_t* score_out, uint8_t* founds, int64_t* indices, hipStream_t stream);

/* table_insert / table_insert_and_evict (+ table_unlock_kernel), src/table_operation/insert.cu:36-45,
 * insert_and_evict.cu:81-93, kernels.cuh:189-585.  Keys must be unique (scored_hashtable.py:148).
 * num_evicted == NULL -> plain insert; otherwise the evicted (key, index, score, table_id) streams are
 * compacted (arbitrary order) and *num_evicted (device int64) counts them.
 * skip (nullable uint8[n]): keys with skip[i] != 0 are ignored (indices[i] untouched). */
int mi355_table_insert(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                       int64_t num_scores, int32_t* bucket_sizes, int32_t* counter, int64_t n,
                       const int64_t* n_dev, const void* keys, const int64_t* table_ids, const void* score_in,
                       int policy, uint64_t timer_override, const uint8_t* skip, int64_t* indices,
                       uint8_t* results, int64_t* score_out, int64_t* num_evicted, void* evicted_keys,
                       int64_t* evicted_indices, int64_t* evicted_scores, int64_t* evicted_table_ids,
                       hipStream_t stream);

/* table_erase, src/table_operation/erase.cu + table_erase_kernel kernels.cuh:587-652 */
int mi355_table_erase(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                      int64_t num_scores, int32_t* bucket_sizes, int64_t n, const void* keys,
                      const int64_t* table_ids, int64_t* indices, hipStream_t stream);

/* table_export_batch, src/table_operation/export_batch.cu:22-124 (kernel kernels.cuh:655-705): the valid slots of
 * [offset, offset+batch) whose score[score_index] >= threshold (has_threshold) -> compacted (keys, scores,
 * indices = slot - table_begin), *counter = how many.  Output is in slot order (the reference: atomic order). */
int64_t mi355_table_export_batch_workspace_bytes(int64_t batch);
int mi355_table_export_batch(const void* storage, int64_t num_buckets, int64_t bucket_capacity, int64_t num_scores,
                             int64_t batch, int64_t offset, int has_threshold, uint64_t threshold,
                             int64_t table_begin, int64_t score_index, int64_t* counter, void* keys,
                             int64_t* scores, int64_t* indices, void* workspace, int64_t workspace_bytes,
                             hipStream_t stream);

/* table_count_matched, src/table_operation/count_matched.cu:23-93: number of valid slots in [begin, end)
 * (negative = whole table) with score[score_index] >= threshold (unsigned compare) -> *num_matched. */
int mi355_table_count_matched(const void* storage, int64_t num_buckets, int64_t bucket_capacity, int64_t num_scores,
                              uint64_t threshold, int64_t begin, int64_t end, int64_t score_index,
                              int64_t* num_matched, hipStream_t stream);

/* table_{copy,gather,scatter}_score_blocks, src/table_operation/insert.cu:155-254 (kernels.cuh:839-910):
 * mode 0 copy src[src_slots]->dst[dst_slots], 1 gather src[src_slots]->dense [n, num_scores], 2 scatter
 * dense->dst[dst_slots]; slots are table-relative, *_bkt_begin the table's first bucket; slot < 0 skipped
 * (gather writes zeros). */
int mi355_table_score_blocks(int mode, const void* src_storage, int64_t src_bucket_capacity, int64_t src_bkt_begin,
                             void* dst_storage, int64_t dst_bucket_capacity, int64_t dst_bkt_begin,
                             int64_t num_scores, int64_t n, const int64_t* src_slots, const int64_t* dst_slots,
                             int64_t* dense, hipStream_t stream);

/* table_update_counter_with_layout, insert_and_evict.cu:27-58,397-430 (main-table region) */
int mi355_table_update_counter(int32_t* counter, int64_t counter_numel, const int64_t* slot_indices, int64_t n,
                               const int64_t* n_dev, int32_t delta, const int64_t* table_ids,
                               const int64_t* table_bucket_offsets, int64_t bucket_capacity, hipStream_t stream);

/* ---- overflow region of cache tables (scored_hashtable.py:426-474, DynamicEmbCache key_value_table.py:1522-1590).
 * ovf_storage: a second table arena with ONE bucket of ovf_capacity (= 3 x bucket_capacity) slots per logical table
 * (same SoA layout, mi355_table_init(ovf_storage, num_tables, ovf_capacity, num_scores)); ovf_bucket_sizes int32[T];
 * ovf_counter int32[T * ovf_capacity] (the tail of the ref-counter array); ovf_output_offsets int64[T] = main capacity
 * of each table: an overflow entry's table-relative index is ovf_output_offsets[t] + position.
 *
 * table_lookup with ovf_storage (lookup.cu:82-150, kernels.cuh:153-183,711-736): keys the main table does not hold are
 * searched in their table's overflow bucket (linear probing from hash % ovf_capacity, stops at Empty). */
int mi355_table_lookup_overflow(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                                int64_t num_scores, int64_t n, const int64_t* n_dev, const void* keys,
                                const int64_t* table_ids, const void* score_in, int policy, uint64_t timer_override,
                                void* ovf_storage, int64_t ovf_capacity, const int64_t* ovf_output_offsets,
                                int64_t* score_out, uint8_t* founds, int64_t* indices, hipStream_t stream);

/* table_insert_and_evict with counter and overflow (insert_and_evict.cu:201-395, kernels.cuh:389-566,738-800): keys whose
 * main bucket is entirely pinned (result Busy) find-or-insert in the overflow bucket; its victims are entries with
 * ref-counter 0.  `results` is required (Insert / Evict / Assign name overflow successes too; compare the index with
 * ovf_output_offsets to tell the regions apart).  Evicted stream as mi355_table_insert: a main-table eviction reports
 * (victim key, its slot), an overflow eviction (victim key, overflow index), a key nobody took (key, -(i+1)).
 * workspace: mi355_table_insert_overflow_workspace_bytes(n). */
int64_t mi355_table_insert_overflow_workspace_bytes(int64_t n);
int mi355_table_insert_overflow(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                                int64_t num_scores, int32_t* bucket_sizes, int32_t* counter, int64_t n,
                                const int64_t* n_dev, const void* keys, const int64_t* table_ids, const void* score_in,
                                int policy, uint64_t timer_override, const uint8_t* skip, void* ovf_storage,
                                int64_t ovf_capacity, int32_t* ovf_bucket_sizes, int32_t* ovf_counter,
                                const int64_t* ovf_output_offsets, int64_t* indices, uint8_t* results, int64_t* score_out,
                                int64_t* num_evicted, void* evicted_keys, int64_t* evicted_indices,
                                int64_t* evicted_scores, int64_t* evicted_table_ids, void* workspace,
                                int64_t workspace_bytes, hipStream_t stream);

/* table_update_counter_with_layout with the overflow layout (insert_and_evict.cu:27-58): slot < ovf_output_offsets[t]
 * -> counter[table_bucket_offsets[t]*C + slot], else counter[main_capacity + t*ovf_capacity + slot - offsets[t]]. */
int mi355_table_update_counter_overflow(int32_t* counter, int64_t counter_numel, const int64_t* slot_indices, int64_t n,
                                        const int64_t* n_dev, int32_t delta, const int64_t* table_ids,
                                        const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                                        int64_t main_capacity, const int64_t* ovf_output_offsets, int64_t ovf_capacity,
                                        hipStream_t stream);

/* device_timestamp, src/torch_utils.cu:22-40,150 */
int mi355_device_timestamp(int64_t* out, hipStream_t stream);

/* ------------------------------------------------------------------------ index ops ---- */

/* segmented_unique_cuda, src/unique_op.cu:484-714.  Outputs sized n; table_offsets[T] is the number
 * of uniques (device).  Unique order = first occurrence inside each table (deterministic). */
int64_t mi355_segmented_unique_workspace_bytes(int64_t n);
int mi355_segmented_unique(const void* keys, int64_t n, const int64_t* segmented_range, int64_t num_tables,
                           const int64_t* input_frequencies, int count_freq, void* unique_keys,
                           int64_t* output_indices, int64_t* table_offsets, int64_t* freq, void* workspace,
                           int64_t workspace_bytes, hipStream_t stream);
/* Same, and (both nullable) csr_cnt int32[n]: occurrences of unique key u in the batch; csr_rank int32[n]: position of
 * occurrence i inside the list of its unique key (a permutation of 0..cnt-1 per key, order unspecified).  They let
 * mi355_group_by_unique_csr build the backward's CSR with a scan and a scatter -- no histogram pass, no atomics. */
int mi355_segmented_unique_csr(const void* keys, int64_t n, const int64_t* segmented_range, int64_t num_tables,
                               const int64_t* input_frequencies, int count_freq, void* unique_keys,
                               int64_t* output_indices, int64_t* table_offsets, int64_t* freq, int32_t* csr_cnt,
                               int32_t* csr_rank, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* expand_table_ids_cuda, src/unique_op.cu:719-750 */
int mi355_expand_table_ids(const int64_t* offsets, int64_t num_tables, int64_t n, const int64_t* n_dev,
                           int64_t* table_ids, hipStream_t stream);

/* get_table_range, src/index_calculation.cu:77-127: range[t] = offsets[feature_offsets[t] * B] with
 * B = feature_x_batch / feature_offsets[T] computed on the device (feature_x_batch = len(offsets) - 1) */
int mi355_get_table_range(const int64_t* offsets, const int64_t* feature_offsets, int64_t num_tables,
                          int64_t feature_x_batch, int64_t* table_range, hipStream_t stream);

/* INFERENCE_EMB::expand_table_ids, src/table_operation/expand_table_ids_torch_binding.cu:17-85: table_ids[i] = the largest
 * t in [0, num_tables] with offsets[fo[t] * local_batch_size] <= i, fo = table_offsets_in_feature (int64[num_tables+1]) or the
 * identity when it is NULL; then num_tables = (offsets_numel - 1) / local_batch_size, as the reference derives it. */
int mi355_inference_expand_table_ids(const int64_t* offsets, int64_t offsets_numel, const int64_t* table_offsets_in_feature,
                                     int64_t num_tables, int64_t local_batch_size, int64_t n, int64_t* table_ids,
                                     hipStream_t stream);

/* InferenceEmbeddingCollection.forward, dynamicemb/exportable_tables.py:501-564 (expand_table_ids + table_lookup under
 * ScorePolicy.CONST + index_select / add + NVEmbedding / NVEmbeddingBag) as ONE read-only launch without a host sync.
 * keys: 8-byte words [n]; offsets [offsets_numel]: CSR offsets of the feature slots; feature_offsets int64[num_tables+1] (NULL:
 * identity); table arena: single-score LinearBucketTable storage (17 bytes per slot) with its table_bucket_offsets, read when
 * use_dynamic_hash != 0 (bucket_capacity a power of two); otherwise a key is its own table-relative index.
 * weight [rows, dim] of weight_dtype (0 fp32, 2 fp16): table t owns rows table_offsets[t] - 1 (its all-zero row, where unknown
 * keys, out-of-range identity keys and out-of-range slots land) .. table_offsets[t + 1] - 2.
 * pooling_mode -1: out [n, dim], a copy of the rows.  1 / 2: out [num_bags, dim] = sum / mean over pooling_offsets
 * (int64[num_bags+1]) with fp32 accumulation in key order, optional per_sample_weights fp32[n] (sum only); out has weight_dtype. */
int mi355_inference_emb_forward(const void* keys, int64_t n, const int64_t* offsets, int64_t offsets_numel,
                                const int64_t* feature_offsets, int64_t num_tables, int64_t local_batch_size,
                                const void* table_storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                                const int64_t* table_offsets, const void* weight, int64_t dim, int weight_dtype,
                                const int64_t* pooling_offsets, int64_t num_bags, const float* per_sample_weights,
                                int pooling_mode, int use_dynamic_hash, void* out, hipStream_t stream);

/* flagged_compact, src/index_calculation.cu:129-232 -- order preserving; the count stays on the
 * device in *count_out (the reference syncs the host here).  Arrays are 8-byte words. */
int64_t mi355_flagged_compact_workspace_bytes(int64_t n);
int mi355_flagged_compact(const uint8_t* flags, int64_t n, const int64_t* n_dev, int64_t* count_out,
                          int64_t* out_index, int num_arrays, const void* const* inputs, void* const* outputs,
                          void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Groups the keys of a batch by unique row (counting sort keyed by the reverse index): stands in for
 * generate_gather_ids_pooled_kernel + cub::DeviceRadixSort of reduce_grads, dynamic_emb_op.cu:140-263.
 * ptr: int32[max_unique+1], csr_src: int32[n] = bag id f*B+b (offsets != NULL) or key position. */
int64_t mi355_group_by_unique_workspace_bytes(int64_t n, int64_t max_unique);
int64_t mi355_hot_rows_workspace_bytes(int64_t num_keys, int64_t dim);
/* hot_workspace (nullable, mi355_hot_rows_workspace_bytes(n, dim) bytes): receives the task list of the
 * rows with more than 16 occurrences; hand the SAME buffer to mi355_backward_fused as `workspace`. */
int mi355_group_by_unique(const int64_t* reverse_indices, int64_t n, const int64_t* offsets, int64_t num_bags,
                          int64_t max_unique, const int64_t* nu_dev, int32_t* ptr, int32_t* csr_src,
                          void* workspace, int64_t workspace_bytes, void* hot_workspace,
                          int64_t hot_workspace_bytes, int64_t dim, hipStream_t stream);
int64_t mi355_group_by_unique_csr_workspace_bytes(int64_t max_unique);
int mi355_group_by_unique_csr(const int32_t* csr_cnt, const int32_t* csr_rank, const int64_t* reverse_indices, int64_t n,
                              const int64_t* offsets, int64_t num_bags, int64_t max_unique, const int64_t* nu_dev,
                              int32_t* ptr, int32_t* csr_src, void* workspace, int64_t workspace_bytes,
                              void* hot_workspace, int64_t hot_workspace_bytes, int64_t dim, hipStream_t stream);

/* block_bucketize_sparse_features, src/sparse_block_bucketize_features.cu:220-350,366-830:
 * dist_type per feature 0 continuous / 1 roundrobin / 2 hash_roundrobin; offsets has num_bags+1 entries
 * (feature-major F*B bags); new_lengths [W*num_bags], new_offsets [W*num_bags+1]. */
int mi355_block_bucketize(int64_t world_size, int64_t num_bags, int64_t batch_size, const int64_t* offsets,
                          const void* indices, const int64_t* block_sizes, const int32_t* dist_type_per_feature,
                          const float* weights, int64_t* new_lengths, int64_t* new_offsets, void* new_indices,
                          float* new_weights, int64_t* unbucketize_permute, hipStream_t stream);
/* The same op with the two remaining arguments of the reference's signature (sparse_block_bucketize_features.cu:366-380):
 * `batch_size_per_feature` -- passed as feature_bag_starts [num_features + 1], the first bag of every feature (its exclusive
 * prefix sum; nullptr: every feature has batch_size bags) -- and `block_bucketize_pos` -- uneven shard boundaries, the sorted
 * boundaries of all features concatenated plus their offsets [num_features + 1] (:262-292, 341-347: rank = last boundary <= idx,
 * new index = idx - that boundary; indices outside the boundaries: idx % W, idx / W; the dist types do not apply). */
int mi355_block_bucketize_ex(int64_t world_size, int64_t num_bags, int64_t batch_size, const int64_t* offsets,
                             const void* indices, const int64_t* block_sizes, const int32_t* dist_type_per_feature,
                             const float* weights, int64_t* new_lengths, int64_t* new_offsets, void* new_indices,
                             float* new_weights, int64_t* unbucketize_permute, const int64_t* feature_bag_starts,
                             int64_t num_features, const int64_t* block_bucketize_pos_concat,
                             const int64_t* block_bucketize_pos_offsets, hipStream_t stream);

/* Glue of the row-wise input dist (dynamicemb/input_dist.py :199-285 + TorchRec KJTAllToAll, third party): exclusive
 * offsets of a lengths vector (offsets has n+1 entries); the keys sent to / received from every peer as differences of
 * the send / receive offsets at the peer boundaries (`splits` [2*W]: send then receive; may be pinned host memory --
 * it is the one host read of the exchange); pseudo-bags of at most `chunk` keys over per-table unique-key lists for
 * the pre-communication dedup (shard/embedding.py:183-275), lengths [T*num_chunks], offsets [T*num_chunks+1]. */
int mi355_exclusive_offsets(const int64_t* lengths, int64_t n, int64_t* offsets, hipStream_t stream);
int mi355_peer_splits(const int64_t* send_offsets, const int64_t* recv_offsets, int64_t bags_per_peer, int64_t world_size,
                      int64_t* splits, hipStream_t stream);
int mi355_chunk_bags(const int64_t* unique_offsets, int64_t num_tables, int64_t chunk, int64_t num_chunks, int64_t* lengths,
                     int64_t* offsets, hipStream_t stream);

/* compute_dedup_lengths_cuda, src/unique_op.cu:753-789 (kernel lookup_kernel.cuh:1049-1090): lengths/offsets that
 * spread each table's unique keys evenly over its (feature, batch) bags.  new_offsets has new_lengths_size+1. */
int mi355_compute_dedup_lengths(const int64_t* unique_offsets, const int64_t* table_offsets_in_feature,
                                int64_t num_tables, int64_t local_batch_size, int64_t new_lengths_size,
                                int64_t* new_lengths, int64_t* new_offsets, hipStream_t stream);

/* segmented_sum_cuda, src/index_calculation.cu:38-75: int32 data, int64 offsets [S+1] -> int64 sums [S]. */
int mi355_segmented_sum(const int32_t* data, const int64_t* offsets, int64_t num_segments, int64_t* out,
                        hipStream_t stream);

/* Bag re-ordering of a received key stream, (source rank, feature, batch) -> (feature, source rank, batch):
 * the recat / permute_2D_sparse_data step of TorchRec's KJTAllToAll (third party), call site
 * dynamicemb/input_dist.py:239-285.  Offsets are exclusive scans of the respective lengths. */
int mi355_permute_lengths(int64_t num_sources, int64_t num_features, int64_t batch_size, const int64_t* in_lengths,
                          int64_t* out_lengths, hipStream_t stream);
/* elem_bytes: bytes per element of the permuted stream (8 for keys, D*sizeof(T) for embedding rows);
 * num_elements: length of the stream (host value, picks the short-bag or long-bag kernel). */
int mi355_permute_bags(int64_t num_sources, int64_t num_features, int64_t batch_size, int64_t elem_bytes,
                       int64_t num_elements, const int64_t* in_offsets, const int64_t* out_offsets, const void* in_keys,
                       void* out_keys, hipStream_t stream);

/* --------------------------------------------------- exchanges of the row-wise sharded lookup ---- */

/* The collectives of a row-wise (model-parallel) sharded step, driven from INSIDE the library -- one call per stage, RCCL on
 * the HIP streams the caller names (csrc/exchange.hip).  Replaces, for GPU tensors, the c10d call sequence of
 * dynamicemb/input_dist.py:199-285 (RwSparseFeaturesDist -> TorchRec KJTAllToAll: lengths all-to-all, keys all-to-all-v, recat)
 * and of the output dists of planner/rw_sharding.py:85-158 (sequence: rows back), :191-261 (pooled: reduce-scatter of partial
 * sums, here all-to-all + local sum; backward all-gather).  RCCL is bound at run time from the librccl.so the process already
 * holds (torch's): mi355_rw_load_rccl(path).  Rank 0 draws two unique ids (128 bytes each) and hands them to every rank by
 * any means (the module broadcasts them over the existing process group); mi355_rw_create is collective. */
int mi355_rw_load_rccl(const char* librccl_path);
int mi355_rw_unique_id(void* out, int64_t bytes);
int mi355_rw_create(const void* id_input_dist, const void* id_output_dist, int world_size, int rank, void** handle);
int mi355_rw_destroy(void* handle);
/* hang guard of the caller's one-time self-check: aborts both communicators (ncclCommAbort: a collective kernel waiting for a
 * peer that never came returns) and frees the handle without a device synchronisation; the caller continues on the c10d
 * sequence.  No reference counterpart (TorchRec relies on ProcessGroupNCCL's watchdog for the same purpose). */
int mi355_rw_abort(void* handle);
/* input dist, first half, on `stream` (behind what `producer_stream` holds): block_bucketize -> all-to-all of the lengths
 * [W][F*B] -> exclusive offsets of the received lengths -> per-peer key counts into pinned memory.  Arrays as
 * mi355_block_bucketize; recv_lengths [W*F*B], recv_offsets [W*F*B+1].  *ticket names the counts for the second half. */
int mi355_rw_input_begin(void* handle, int64_t num_features, int64_t batch_size, const int64_t* offsets, const void* keys,
                         const int64_t* block_sizes, const int32_t* dist_types, int64_t* new_lengths, int64_t* new_offsets,
                         void* new_keys, int64_t* unbucketize_permute, int64_t* recv_lengths, int64_t* recv_offsets,
                         hipStream_t producer_stream, hipStream_t stream, int* ticket);
/* the one host read of the exact exchange: waits for the launch that wrote the counts; send_splits / recv_splits [W] (host),
 * totals[0] = keys sent, totals[1] = keys received (the size of the buffer mi355_rw_input_keys fills) */
int mi355_rw_input_counts(void* handle, int ticket, int64_t* send_splits, int64_t* recv_splits, int64_t* totals);
/* 1 when mi355_rw_input_counts(ticket) would not wait (the launch that writes the counts has completed), else 0 */
int mi355_rw_input_counts_ready(void* handle, int ticket);
/* second half on `stream`: all-to-all-v of the 8-byte keys, recat to feature-major when W > 1 and F > 1 (fm_* buffers, else
 * unused: the received order IS feature-major); `consumer_stream` (if another stream) is ordered behind it */
int mi355_rw_input_keys(void* handle, int ticket, int64_t num_features, int64_t batch_size, const void* new_keys,
                        void* recv_keys, const int64_t* recv_lengths, const int64_t* recv_offsets, int64_t* fm_lengths,
                        int64_t* fm_offsets, void* fm_keys, hipStream_t stream, hipStream_t consumer_stream);
int mi355_rw_wait_keys(void* handle, int ticket, hipStream_t consumer_stream);
/* 1 when the key exchange of `ticket` has completed on the device, else 0 (an event query, never waits) */
int mi355_rw_keys_ready(void* handle, int ticket);
/* gives a ticket back whose second half will not run (at most 8 input dists may be in flight: a 9th mi355_rw_input_begin
 * before the oldest mi355_rw_input_keys is refused) */
int mi355_rw_input_cancel(void* handle, int ticket);
/* pooled output dist: all-to-all of the W blocks of numel_per_block partial sums (wire_dtype) + their fp32 sum -> out */
int mi355_rw_output_pooled(void* handle, const void* send, void* recv, int64_t numel_per_block, int wire_dtype, void* out,
                           int out_dtype, hipStream_t stream);
/* pooled backward: all-gather of `bytes` bytes per rank */
int mi355_rw_allgather(void* handle, const void* send, void* recv, int64_t bytes, hipStream_t stream);
/* sequence output dist / its backward: all-to-all-v of rows; counts in elements of elem_bytes (host arrays [W]) */
int mi355_rw_alltoallv(void* handle, const void* send, const int64_t* send_counts, void* recv, const int64_t* recv_counts,
                       int64_t elem_bytes, hipStream_t stream);

/* ------------------------------------------------------------------------ value ops ---- */

/* out[r] = sum_c in[c][r] (fp32 partial pooled sums of the W shards -> output dtype): the local half of the
 * pooled output dist (TorchRec RwPooledEmbeddingSharding reduce-scatter, planner/rw_sharding.py:191-261). */
int mi355_sum_chunks(const float* in, int64_t chunks, int64_t numel_per_chunk, void* out, int out_dtype,
                     hipStream_t stream);
/* the same for chunks in a 16-bit wire type (TorchRec's qcomm codec on the reduce-scatter: the shards' partial sums cross the
 * fabric in bf16 / fp16, fbgemm_gpu quantize_comm; here the sum reads them directly, fp32 accumulation) */
int mi355_sum_chunks_typed(const void* in, int in_dtype, int64_t chunks, int64_t numel_per_chunk, void* out, int out_dtype,
                           hipStream_t stream);
/* the same with chunk `self_index` read from `self_chunk` instead of `in` (the rank's own block stays where the lookup wrote it:
 * it does not travel through the all-to-all); sum order unchanged */
int mi355_sum_chunks_self(const void* in, int in_dtype, int64_t chunks, int64_t numel_per_chunk, const void* self_chunk,
                          int64_t self_index, void* out, int out_dtype, hipStream_t stream);


/* gather_embedding_pooled, src/dynamic_emb_op.cu:106-133 (kernels lookup_kernel.cuh:859-998).
 * Source: dense [*, src_stride] (reference form) or table rows through row_addr[u] (fused form;
 * address 0 = missing row = zeros).  offsets feature-major [num_bags+1]; combiner 0 sum / 1 mean;
 * D_offsets (int32[F+1]) NULL for uniform dim.  aligned16: rows, dims and column offsets allow
 * 4-element vector access. */
int mi355_gather_pooled(const void* src, int64_t src_stride, const int64_t* row_addr, int src_dtype,
                        const int64_t* reverse_indices, int64_t num_keys, const int64_t* offsets, int64_t num_bags,
                        int64_t batch_size, int combiner, int64_t dim, const int32_t* D_offsets, int64_t total_D,
                        void* dst, int dst_dtype, int aligned16, hipStream_t stream);

/* gather_embedding, src/dynamic_emb_op.cu:79-104 (index NULL = identity) */
int mi355_gather_rows(const void* src, int64_t src_stride, const int64_t* row_addr, int src_dtype,
                      const int64_t* index, int64_t n, const int64_t* n_dev, int64_t dim, void* dst,
                      int64_t dst_stride, int dst_dtype, int aligned16, hipStream_t stream);

/* load_from_flat_table_{contiguous,emb,value} (is_load=1) / store_to_flat_table_{contiguous,value}
 * (is_load=0), src/dynamic_emb_op.cu:294-684.  region 0/1/2 as NumRegions there. */
int mi355_flat_table_copy(int is_load, int region, int64_t n, const int64_t* n_dev, void* dense,
                          int64_t dense_dim, int64_t dense_stride, int dtype, const int64_t* indices,
                          const int64_t* table_ids, int64_t scalar_table_id, const int64_t* table_ptrs,
                          const int64_t* table_value_dims, const int64_t* table_emb_dims, int64_t max_emb_dim,
                          hipStream_t stream);

/* row_addr[u] = table_ptrs[tid] + slot * value_dim * elem_bytes (0 for slot < 0): the address form of
 * the (table_ptrs, table_ids, indices) triple every flat-table kernel of the reference takes. */
int mi355_row_addresses(int64_t n, const int64_t* n_dev, const int64_t* slots, const int64_t* table_ids,
                        const int64_t* table_ptrs, const int64_t* table_value_dims, int elem_bytes,
                        int64_t* row_addr, hipStream_t stream);

/* {uniform,normal,truncated_normal,const,debug}_init, src/initializer.cu:64-212.  mode 0..4. */
int mi355_init_rows(int mode, float p0, float p1, float p2, float p3, uint64_t seed, float state_init,
                    int64_t n, const int64_t* n_dev, const void* keys, const int64_t* sel,
                    const int64_t* row_addr, void* dense, int64_t dense_stride, int dtype, int64_t emb_dim,
                    int64_t value_dim, const uint8_t* results, const uint8_t* skip, const int64_t* table_ids,
                    const int64_t* table_emb_dims, const int64_t* table_value_dims, hipStream_t stream);

/* ------------------------------------------------------------------------- backward ---- */

/* reduce_grads (opt_kind 0, src/dynamic_emb_op.cu:159-285) and reduce_grads fused with
 * {sgd,adam,adagrad,rowwise_adagrad}_update_for_flat_table (opt_kind 1..4, src/optimizer.cu:77-240)
 * over the CSR of mi355_group_by_unique.  combiner -1 sequence / 0 sum / 1 mean.
 * opt_kind 0 writes the reduced gradients to `out` [max_unique, out_stride] and `weight_dtype` is then the dtype
 * of `out` (the reference returns the grad dtype; fp32 keeps the sums exact for the sharded backward). */
int64_t mi355_backward_workspace_bytes(int64_t num_keys, int64_t dim);
int mi355_backward_fused(const int32_t* ptr, const int32_t* csr_src, int64_t num_keys, int64_t max_unique,
                         const int64_t* nu_dev, const void* grads, int64_t grad_stride, int grad_dtype,
                         const int64_t* offsets, const int32_t* D_offsets, int64_t batch_size, int64_t dim,
                         int combiner, const int64_t* row_addr, int weight_dtype, int opt_kind, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int64_t iter_num,
                         int64_t state_offset, int round_grad, void* out, int64_t out_stride, int aligned16,
                         void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* {sgd,adam,adagrad,rowwise_adagrad}_update_for_flat_table (row_addr) / ..._for_padded_buffer
 * (dense_rows), src/optimizer.cu:77-476, on dense unique gradients. */
int mi355_optimizer_update(int opt_kind, const void* grads, int64_t grad_stride, int grad_dtype, int64_t n,
                           const int64_t* n_dev, const int64_t* row_addr, void* dense_rows, int64_t dense_stride,
                           int weight_dtype, int64_t dim, int64_t state_offset, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int64_t iter_num, int aligned16,
                           hipStream_t stream);
/* the padded-buffer form over rows of tables with DIFFERENT embedding widths (update4_padded_buffer_kernel,
 * src/optimizer_kernel.cuh:473-493): row u is table_emb_dims[table_ids[u]] wide, its optimizer state starts at state_offset
 * (= the widest embedding) whatever its own width; table_ids == nullptr: every row is `dim` wide (the entry above). */
int mi355_optimizer_update_tables(int opt_kind, const void* grads, int64_t grad_stride, int grad_dtype, int64_t n,
                                  const int64_t* n_dev, const int64_t* row_addr, void* dense_rows, int64_t dense_stride,
                                  int weight_dtype, int64_t dim, int64_t state_offset, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, int64_t iter_num, int aligned16, const int64_t* table_ids,
                                  const int64_t* table_emb_dims, hipStream_t stream);

/* ---------------------------------------------------------------- growable buffers ---- */

/* VMMTensor / HostVMMTensor (src/vmm_tensor.cu:30-585, pybind :555-585): a buffer that grows IN PLACE.  Address space for
 * `reserve_bytes` is reserved once; `initial_bytes` (then every mi355_vmm_extend) maps zero-filled physical memory at the
 * tail -- HBM through hipMemCreate / hipMemMap for host == 0, pinned host memory (mmap + hipHostRegister, addressable by
 * the kernels through the same pointer) for host != 0.  The data pointer never changes. */
int mi355_vmm_create(int64_t reserve_bytes, int64_t initial_bytes, int device, int host, void** handle_out);
int mi355_vmm_extend(void* handle, int64_t new_total_bytes);
void* mi355_vmm_data(void* handle);
int64_t mi355_vmm_mapped_bytes(void* handle);
int64_t mi355_vmm_reserved_bytes(void* handle);
int mi355_vmm_destroy(void* handle);

/* ------------------------------------------------------------------ fused pipelines ---- */

/* One-call forward of BatchedDynamicEmbeddingTablesV2 with HBM-only storage:
 * dynamicemb_prefetch (_prefetch_hbm_direct_path) + DynamicEmbeddingFunction.forward, or
 * dynamicemb_eval_forward when train == 0 (dynamicemb/batched_dynamicemb_function.py:559-932,1042-1191).
 * No host sync; persisted arrays feed mi355_demb_backward. */
int64_t mi355_demb_forward_workspace_bytes(int64_t num_keys, int64_t num_tables);
int mi355_demb_forward(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                       int64_t num_scores, int32_t* bucket_sizes, int32_t* counter, int64_t counter_numel,
                       const int64_t* table_ptrs, const int64_t* table_value_dims, const int64_t* table_emb_dims,
                       int value_dtype, int64_t emb_dim, int64_t value_dim, const void* keys, int64_t num_keys,
                       const int64_t* offsets, int64_t num_bags, int64_t batch_size, const int64_t* feature_offsets,
                       int64_t num_tables, int train, int find_policy, const void* find_scores, int insert_policy,
                       const void* insert_scores, uint64_t timer_override, int pin, int init_mode, float p0,
                       float p1, float p2, float p3, uint64_t seed, float state_init, int combiner,
                       const int32_t* D_offsets, int64_t total_D, void* out, int out_dtype, int aligned16,
                       int64_t* reverse_indices, int64_t* unique_offsets, int64_t* table_ids, int64_t* slots,
                       int64_t* row_addr, int64_t* freq, int32_t* csr_cnt /* nullable */,
                       int32_t* csr_rank /* nullable */,
                       void* backward_workspace /* nullable: early CSR, see mi355_demb_backward(prepared) */,
                       int64_t backward_workspace_bytes,
                       int* join_token /* out, nullable: side-stream join point of the early CSR (-1: none) */,
                       void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* The same step with the index stage FUSED into one kernel (csrc/fused_fwd.hip): tile dedup in LDS, hash-table probe of
 * the tile's distinct keys, per-slot occurrence counting (dedup BY SLOT), in-place insert + first-touch initialisation of
 * unseen keys, deferred min-score eviction for full buckets -- segmented_unique_cuda (src/unique_op.cu:484-714) +
 * table_lookup / table_insert / table_unlock (src/table_operation/kernels.cuh:81-585) + initializer + the pin bracket of
 * _prefetch_hbm_direct_path (dynamicemb/batched_dynamicemb_function.py:559-696) in ONE launch; the pooled / sequence
 * gather reads per-occurrence row addresses and the unique numbering + the backward's CSR run on the library's side
 * stream (use_side_stream) under it.  `aux`: persistent int32 scratch of mi355_demb_aux_numel() elements owned by the
 * table, zero-initialised once by the caller and left all-zero by every call.  Scores are scalar: `score_value`, or the
 * per-key occurrence count when use_count != 0 (LFU).  Unique keys come out in representative order (not first
 * occurrence); in eval mode (train == 0) only `out` is produced.  join_token as in mi355_demb_forward. */
int64_t mi355_demb_aux_numel(int64_t total_slots, int64_t num_buckets);
/* measurement hook of bench.py: while enabled, the library brackets the launches of its two bandwidth kernels with HIP
 * events on the launch stream; mi355_profile_ms(slot) returns the duration of the last one (-1: none) */
int mi355_profile_kernels(int enable);
float mi355_profile_ms(int slot /* 0: gather of the fused forward, 1: backward kernel */);
/* `stream` waits for the side-stream work a forward announced through join_token */
int mi355_side_join(int token, hipStream_t stream);
/* Slot-range partitions the fused forward uses for a training batch of n keys (0: the per-slot-counter path).  One table,
 * 64 K .. 1 M keys and at least 8 buckets per partition take the partitioned index stage: (tile, key) records grouped by
 * slot range, one block per range merges them in LDS -- no global atomic per key, no per-slot scratch. */
int mi355_demb_forward_fused_partitions(int64_t n, int64_t num_tables, int64_t num_buckets);

/* Per-key frequency weights (the reference's per_sample_weights / frequency_counters: counts, not pooling weights).  Binds
 * `weights` (int64 [num_keys], device) to the NEXT index stage the calling thread issues -- mi355_demb_forward,
 * mi355_demb_forward_fused(_rerun), mi355_demb_plan_forward / _stage / _rerun --, which consumes the binding; a plan call that
 * returns MI355_ENOSPC (nothing launched) keeps it.  A counting score policy (Accumulate; LRU_LFU's frequency word), the insert of
 * an unseen key and the admission counter then add the SUM of a key's weights where they add its occurrence count otherwise.
 * Outputs, gradients, the other score policies and eval forwards do not see them.  Negative weights are the caller's error.
 * workspace: mi355_demb_weights_workspace_bytes(num_keys, num_tables) bytes of device scratch, untouched until the bound call's
 * kernels have run. */
int64_t mi355_demb_weights_workspace_bytes(int64_t num_keys, int64_t num_tables);
int mi355_demb_bind_weights(const int64_t* weights, int64_t num_keys, void* workspace, int64_t workspace_bytes);
/* Round 3: a pooled training forward of the partitioned stage (path (c), MI355_FUSED_PART=2) returns *join_token == -2.  Its
 * partition kernel wrote the backward's CSR itself (no scatter kernel); the per-occurrence outputs nothing on the training path reads --
 * reverse_indices (the `inverse` of segmented_unique_cuda, src/unique_op.cu:484-714) and csr_rank -- are produced by this call
 * on demand, from the step's forward workspace (untouched since the forward). */
int mi355_demb_fused_materialize(void* workspace, int64_t workspace_bytes, int64_t num_keys, int64_t num_tables,
                                 const int64_t* row_addr, int64_t* reverse_indices, int32_t* csr_rank, hipStream_t stream);
int64_t mi355_demb_forward_fused_workspace_bytes(int64_t num_keys, int64_t num_tables);
int mi355_demb_forward_fused(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                             int64_t num_scores, int32_t* bucket_sizes, int32_t* counter, int64_t counter_numel,
                             int32_t* aux, int64_t aux_numel, int64_t num_buckets, const int64_t* table_ptrs,
                             const int64_t* table_value_dims, const int64_t* table_emb_dims, int value_dtype,
                             int64_t emb_dim, int64_t value_dim, const void* keys, int64_t num_keys,
                             const int64_t* offsets, int64_t num_bags, int64_t batch_size,
                             const int64_t* feature_offsets, int64_t num_tables, int train, int find_policy,
                             int insert_policy, uint64_t score_value, int use_count, uint64_t timer_override, int pin,
                             int init_mode, float p0, float p1, float p2, float p3, uint64_t seed, float state_init,
                             int combiner, const int32_t* D_offsets, int64_t total_D, void* out, int out_dtype,
                             int aligned16, int64_t* reverse_indices, int64_t* unique_offsets, int64_t* table_ids,
                             int64_t* slots, int64_t* row_addr, int64_t* freq, int32_t* csr_cnt, int32_t* csr_rank,
                             void* backward_workspace, int64_t backward_workspace_bytes, int use_side_stream,
                             int* join_token, void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* Round 6: no step ever loses its update (the reference's unique op serves any key stream in one pass, src/unique_op.cu:484-714;
 * DynamicEmbeddingFunction.backward updates every unique row of every step, batched_dynamicemb_function.py:1193-1300).  Path (c)
 * gives every slot-range partition a fixed record list; a key stream that defeats the hash can flood one.  Such a step's FORWARD
 * output is complete, its CSR is not.  A path-(c) training forward therefore returns *join_token = -(2 + epoch), epoch > 0: its
 * partition kernel stores {epoch, flooded} into pinned host memory as its first action, and the caller asks
 * mi355_demb_fused_step_flooded(epoch, wait_ms) before it uses the step's CSR or unique numbering: 0 = complete; 1 (or 2: the
 * notice was overwritten 64 steps later, treated alike) = flooded: run mi355_demb_forward_fused_rerun (the arguments of the step's
 * forward call + its epoch; `out` untouched), which regroups the step on the per-slot-counter path over the same buffers, then
 * the backward as usual; -1 = the forward has not reached its partition kernel within wait_ms; 3 = a gather block of a
 * sequence lookup abandoned its bounded wait for a partition block of the same launch (the output lacks rows: an error).  The steady state pays one host
 * read of pinned memory per step and no launch.  *join_token == -2 (a forward captured into a hipGraph, pin != 0, or
 * MI355_FUSED_OVERFLOW_RERUN=1): the re-run chain rode behind the gather in the same call, gated on the device; nothing to ask. */
int mi355_demb_fused_step_flooded(int epoch, int wait_ms);
int mi355_demb_forward_fused_rerun(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                                   int64_t num_scores, int32_t* bucket_sizes, int32_t* counter, int64_t counter_numel,
                                   int32_t* aux, int64_t aux_numel, int64_t num_buckets, const int64_t* table_ptrs,
                                   const int64_t* table_value_dims, const int64_t* table_emb_dims, int value_dtype,
                                   int64_t emb_dim, int64_t value_dim, const void* keys, int64_t num_keys,
                                   const int64_t* offsets, int64_t num_bags, int64_t batch_size,
                                   const int64_t* feature_offsets, int64_t num_tables, int train, int find_policy,
                                   int insert_policy, uint64_t score_value, int use_count, uint64_t timer_override, int pin,
                                   int init_mode, float p0, float p1, float p2, float p3, uint64_t seed, float state_init,
                                   int combiner, const int32_t* D_offsets, int64_t total_D, void* out, int out_dtype,
                                   int aligned16, int64_t* reverse_indices, int64_t* unique_offsets, int64_t* table_ids,
                                   int64_t* slots, int64_t* row_addr, int64_t* freq, int32_t* csr_cnt, int32_t* csr_rank,
                                   void* backward_workspace, int64_t backward_workspace_bytes, int use_side_stream,
                                   int epoch, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* Round 5: the pre-bound training step.  Replaces, for the steady-state training step, the per-call argument marshalling of
 * DynamicEmbeddingFunction.forward / backward (batched_dynamicemb_function.py:1042-1300), which re-reads the constructor state of
 * BatchedDynamicEmbeddingTablesV2 (batched_dynamicemb_tables.py:462-787, 999-1088) on every step: a plan holds the table, value
 * buffers, policies, initializer and optimizer of ONE module; a step is then plan_forward(batch, out, step buffer) +
 * plan_backward(step buffer, grads).  The step buffer holds the persisted arrays of mi355_demb_forward_fused and both
 * workspaces; mi355_demb_step_layout is the only definition of its layout (13 int64: ten offsets -- rev, tids, slots, row_addr,
 * freq, csr_cnt, csr_rank, unique_offsets, forward workspace, backward workspace --, total bytes, the two workspace sizes).
 * plan_forward returns 1 (nothing launched) when the buffer is smaller than mi355_demb_plan_step_bytes(num_keys). */
void* mi355_demb_plan_create(void* storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity, int64_t num_scores,
                             int32_t* bucket_sizes, int32_t* counter, int64_t counter_numel, int32_t* aux, int64_t aux_numel,
                             int64_t num_buckets, const int64_t* table_ptrs, const int64_t* table_value_dims,
                             const int64_t* table_emb_dims, int value_dtype, int64_t emb_dim, int64_t value_dim,
                             const int64_t* feature_offsets, int64_t num_tables, int find_policy, int insert_policy,
                             int use_count, int pin, int init_mode, float p0, float p1, float p2, float p3, uint64_t seed,
                             float state_init, int combiner, const int32_t* D_offsets, int64_t total_D, int out_dtype,
                             int aligned16, int opt_kind, float beta1, float beta2, float eps, float weight_decay);
void mi355_demb_plan_destroy(void* plan);
void mi355_demb_step_layout(int64_t num_keys, int64_t num_tables, int64_t dim, int train, int64_t* out13);
int64_t mi355_demb_plan_step_bytes(void* plan, int64_t num_keys);
int mi355_demb_plan_forward(void* plan, const void* keys, int64_t num_keys, const int64_t* offsets, int64_t num_bags,
                            int64_t batch_size, uint64_t score_value, uint64_t timer_override, void* out, void* step_buf,
                            int64_t step_bytes, int* state, hipStream_t stream);
/* Round 6: the forward in two halves -- the reference's prefetch pipeline (BatchedDynamicEmbeddingTablesV2.prefetch,
 * batched_dynamicemb_tables.py:1090-1137; PrefetchTrainPipelineSparseDist, train_pipeline.py:533-692) on the fast index path.
 * stage 1 = index stage only (issued for batch k + 1 on a side stream under the backward of batch k), stage 2 = the gather of a
 * step whose stage 1 ran earlier, stage 0 = mi355_demb_plan_forward.  protect_score: evictions of this call spare every slot whose
 * score is >= it (what the reference's ref-counter pins achieve; exact for the recency policies STEP / TIMESTAMP).  Returns 3 with
 * nothing launched when the batch is not eligible for the partitioned index path. */
int mi355_demb_plan_stage(void* plan, int stage, uint64_t protect_score, const void* keys, int64_t num_keys, const int64_t* offsets,
                          int64_t num_bags, int64_t batch_size, uint64_t score_value, uint64_t timer_override, void* out,
                          void* step_buf, int64_t step_bytes, int* state, hipStream_t fork_from, int slot, hipStream_t stream);
/* (slot 0..3: the stream order of the staged step is kept by the library -- stage 1 on `stream` starts behind what `fork_from`
 *  holds at the call and marks its end, stage 2 waits for the mark; slot -1: the caller orders its streams itself) */
int mi355_demb_plan_backward(void* plan, void* step_buf, int64_t step_bytes, int64_t num_keys, const int64_t* offsets,
                             int64_t num_bags, int64_t batch_size, const void* grads, int64_t grad_stride, int grad_dtype,
                             int grad_aligned16, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int64_t iter_num, int prepared, int epoch, hipStream_t stream);
/* (epoch > 0: the step's overflow notice is read first; a flooded step returns 2 with nothing launched -- call
 *  mi355_demb_plan_rerun(the batch of the step's plan_forward call, its epoch = -2 - *state) and then plan_backward with epoch 0) */
int mi355_demb_plan_rerun(void* plan, const void* keys, int64_t num_keys, const int64_t* offsets, int64_t num_bags,
                          int64_t batch_size, uint64_t score_value, uint64_t timer_override, void* step_buf,
                          int64_t step_bytes, int epoch, hipStream_t stream);

/* hipStream_t of the library's side stream (early CSR build of mi355_demb_forward); NULL if it cannot be created */
void* mi355_early_csr_stream(void);

/* One-call backward: DynamicEmbeddingFunction.backward (batched_dynamicemb_function.py:1193-1300):
 * reduce_grads + optimizer.fused_update_for_flat_table + decrement_counter.  Early CSR: when the forward was given
 * `backward_workspace`, the key-grouping half of this call already ran on the library's side stream under the forward's
 * own lookup / gather kernels; pass the same buffer with prepared = 2 + join_token (1: the grouping was issued on this
 * very stream, nothing to join) and only the reduce + optimizer kernel remains. */
int64_t mi355_demb_backward_workspace_bytes(int64_t num_keys, int64_t dim);
int mi355_demb_backward(const int64_t* reverse_indices, int64_t num_keys, const int64_t* unique_offsets,
                        int64_t num_tables, const int64_t* offsets, int64_t num_bags, int64_t batch_size,
                        const void* grads, int64_t grad_stride, int grad_dtype, const int32_t* D_offsets,
                        int64_t dim, int combiner, const int64_t* row_addr, int value_dtype, int opt_kind, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int64_t iter_num,
                        int64_t state_offset, int round_grad, int aligned16, int32_t* counter,
                        int64_t counter_numel, const int64_t* slots, const int64_t* table_ids,
                        const int64_t* table_bucket_offsets, int64_t bucket_capacity, int unpin,
                        const int32_t* csr_cnt, const int32_t* csr_rank /* from the forward, or both NULL */,
                        int prepared /* 0 group here; 1 / 2 + token: workspace == the forward's backward_workspace */,
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---------------------------------------------------------------- HSTU jagged attention ---- */

/* hstu_varlen_fwd (corelib/hstu/csrc/hstu_attn/hstu_api.cpp:335-523; torch.ops.fbgemm.hstu_varlen_fwd_80,
 * examples/hstu/ops/fused_hstu_op.py:318-337): out = M * SiLU(alpha q k^T) v / scaling_seqlen per jagged
 * sequence.  q, k, v, out: bf16 [total, H, d], element strides between tokens / heads given explicitly
 * (last dim contiguous); cu_seqlens int32 [batch+1] (shared by q and k); num_contexts / num_targets
 * int32 [batch] or NULL; causal = window (-1, 0), else full (-1, -1); head_dim in {32, 64, 128, 256}. */
int mi355_hstu_attn_fwd(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                        int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                        int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                        const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim,
                        int64_t max_seqlen, const int32_t* num_contexts, const int32_t* num_targets,
                        int64_t target_group_size, int causal, float alpha, float scaling_seqlen,
                        hipStream_t stream);

/* Inference forward of the same op: the queries may be the LAST tokens of a longer key sequence (cu_seqlens_k;
 * the reference's delta-q) and the history keys / values may live in a paged cache [num_pages, 2, page_size, H, d]
 * addressed through (page_offsets [batch+1], page_ids, last_page_lens [batch]) -- hstu_attn_varlen_func(...,
 * kv_cache=, page_offsets=, page_ids=, last_page_lens=) of examples/hstu/modules/paged_hstu_infer_layer.py:492-514,
 * kernel hstu_fwd.h Paged_KV paths :104-131,516-545,785; reference statement _hstu_paged_kv_attention,
 * examples/hstu/test/test_paged_hstu_attn_kernel.py:179-256.  With a cache, k / v hold [new history | candidates]
 * per sequence and only their candidate rows are read (the history, new tokens included, is in the cache);
 * cu_seqlens_k[b+1]-cu_seqlens_k[b] = cached length + num_targets[b].  NULL cu_seqlens_k / kv_cache = training call. */
int mi355_hstu_attn_fwd_kv(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                           int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                           int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                           const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                           int64_t head_dim, int64_t max_seqlen_q, const int32_t* num_contexts,
                           const int32_t* num_targets, int64_t target_group_size, int causal, float alpha,
                           float scaling_seqlen, const void* kv_cache, const int32_t* page_offsets,
                           const int32_t* page_ids, const int32_t* last_page_lens, int64_t page_size,
                           hipStream_t stream);

/* mi355_hstu_attn_fwd_kv under a local attention window (hstu_attn_varlen_func(window_size=(left, right)) with cu_seqlens_k longer
 * than cu_seqlens_q and / or kv_cache; the reference composes Is_local with the delta-q offset and Paged_KV, hstu_fwd.h:104-131,
 * 463-470,516-545): the window runs over absolute positions, query r of a sequence sitting at Lk - Lq + r.  No contextual /
 * target rows (hstu_attn_interface.py:238-245). */
int mi355_hstu_attn_fwd_kv_window(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                                  int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                                  int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                                  const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                                  int64_t head_dim, int64_t max_seqlen_q, int64_t window_left, int64_t window_right,
                                  float alpha, float scaling_seqlen, const void* kv_cache, const int32_t* page_offsets,
                                  const int32_t* page_ids, const int32_t* last_page_lens, int64_t page_size,
                                  hipStream_t stream);
int mi355_hstu_attn_fwd_kv_window_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                                      int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                                      int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                                      const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                                      int64_t head_dim, int64_t max_seqlen_q, int64_t window_left, int64_t window_right,
                                      float alpha, float scaling_seqlen, const void* kv_cache, const int32_t* page_offsets,
                                      const int32_t* page_ids, const int32_t* last_page_lens, int64_t page_size,
                                      hipStream_t stream);

/* mi355_hstu_attn_fwd_kv with a relative attention bias (hstu_attn_varlen_func(rab=...) with cu_seqlens_k longer than
 * cu_seqlens_q and / or kv_cache; hstu_fwd.h:104-131,516-545 with Has_rab): rab [batch][heads or 1][max_seqlen_k][max_seqlen_k]
 * is indexed by ABSOLUTE positions -- query r of a sequence is row Lk - Lq + r.  Mask as window_size: (-1, 0) causal
 * (num_contexts / num_targets allowed), (-1, -1) full, otherwise a local window. */
int mi355_hstu_attn_fwd_kv_rab(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride, int64_t k_row_stride,
                               int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride, int64_t k_head_stride,
                               int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens_q,
                               const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads, int64_t head_dim,
                               int64_t max_seqlen_q, int64_t max_seqlen_k, const int32_t* num_contexts,
                               const int32_t* num_targets, int64_t target_group_size, int64_t window_left,
                               int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                               int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, const void* kv_cache,
                               const int32_t* page_offsets, const int32_t* page_ids, const int32_t* last_page_lens,
                               int64_t page_size, hipStream_t stream);
int mi355_hstu_attn_fwd_kv_rab_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride, int64_t k_row_stride,
                               int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride, int64_t k_head_stride,
                               int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens_q,
                               const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads, int64_t head_dim,
                               int64_t max_seqlen_q, int64_t max_seqlen_k, const int32_t* num_contexts,
                               const int32_t* num_targets, int64_t target_group_size, int64_t window_left,
                               int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                               int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, const void* kv_cache,
                               const int32_t* page_offsets, const int32_t* page_ids, const int32_t* last_page_lens,
                               int64_t page_size, hipStream_t stream);

/* Arbitrary mask functions (`func` of hstu_attn_varlen_func, hstu_api.cpp:170-180; applied per element inside the reference's
 * kernels, hstu_fwd.h:139-145, 493-556 / hstu_bwd.h) read INSIDE the kernels: int32 func[heads or 1][n_func][>= total_q] (n_func
 * odd; head stride 0 = one set for all heads; func_bound_stride = elements between the bounds of a token; last dimension
 * contiguous).  Query token t sees key position j of its sequence iff j < func[0][t] or func[2p-1][t] <= j < func[2p][t], p >= 1;
 * a masked pair gets func_neg (< 0, finite in the operand type: -1e9 bf16, -6e4 fp16) added to q.k, so SiLU and SiLU' are exactly
 * 0 there.  Mask arguments as the *_rab entry points (the other masks apply on top).  Forward: training keys, delta-q keys and
 * the paged cache; backward: self attention over contiguous keys.  No [batch, heads, N, N] tensor exists anywhere. */
int mi355_hstu_attn_fwd_kv_func(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride, int64_t k_row_stride,
                                int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride, int64_t k_head_stride,
                                int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                                int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen_q, int64_t max_seqlen_k,
                                const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                                int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const int32_t* func,
                                int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                                const void* kv_cache, const int32_t* page_offsets, const int32_t* page_ids,
                                const int32_t* last_page_lens, int64_t page_size, hipStream_t stream);
int mi355_hstu_attn_fwd_kv_func_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride, int64_t k_row_stride,
                                int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride, int64_t k_head_stride,
                                int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                                int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen_q, int64_t max_seqlen_k,
                                const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                                int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const int32_t* func,
                                int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                                const void* kv_cache, const int32_t* page_offsets, const int32_t* page_ids,
                                const int32_t* last_page_lens, int64_t page_size, hipStream_t stream);
/* (round 6) func_workspace (nullable): room for the tables of the tile skipping -- 72 bytes x (total_tokens / 128 + batch + 1)
 * per function set (heads, or 1 when the head stride is 0); the reference derives the valid key blocks from the func extents the
 * same way (hstu_fwd.h:80-83, 139-151, 228-291, 411-412).  NULL / too small: the key-major passes visit every query tile.
 * workspace / workspace_bytes (nullable): the P / dS exchange scratch of mi355_hstu_attn_bwd (same sizing calls); used for functions
 * of up to two bands (n_func <= 5) at head_dim 256 when func_workspace is given, otherwise the recomputing passes run. */
int mi355_hstu_attn_bwd_func(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                             int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                             int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                             const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                             const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                             int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const int32_t* func,
                             int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                             void* func_workspace, int64_t func_workspace_bytes, void* workspace, int64_t workspace_bytes,
                             hipStream_t stream);
int mi355_hstu_attn_bwd_func_f16(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                             int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                             int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                             const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                             const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                             int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const int32_t* func,
                             int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                             void* func_workspace, int64_t func_workspace_bytes, void* workspace, int64_t workspace_bytes,
                             hipStream_t stream);

/* Mask functions BESIDE a relative attention bias (hstu_attn_varlen_func(rab=..., func=...); the reference's kernels take the two
 * together, Has_rab x Is_arbitrary), both read inside the kernels: per key tile the row's rab values are added to q.k, then the
 * function test adds func_neg where the row does not see the key.  Key tiles no row of a wave reaches are skipped before their rab
 * row is loaded; no [batch, heads, N, N] mask tensor exists.  With num_contexts the functions narrow the mask except for the history
 * columns of contextual rows.  Arguments: the mask arguments, the four rab arguments and the five func arguments as in
 * mi355_hstu_attn_fwd_kv_rab / mi355_hstu_attn_fwd_kv_func, then the paged cache.  cu_seqlens_k NULL = self attention (training);
 * otherwise delta-q keys and / or the paged cache (rab by absolute positions, func by query token).  Each entry point checks the
 * window, the causal mask, rab (and drab), func, then what every entry point checks. */
int mi355_hstu_attn_fwd_kv_rab_func(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                                    int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                                    int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                                    const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                                    int64_t head_dim, int64_t max_seqlen_q, int64_t max_seqlen_k, const int32_t* num_contexts,
                                    const int32_t* num_targets, int64_t target_group_size, int64_t window_left,
                                    int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                                    int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, const int32_t* func,
                                    int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                                    const void* kv_cache, const int32_t* page_offsets, const int32_t* page_ids,
                                    const int32_t* last_page_lens, int64_t page_size, hipStream_t stream);
int mi355_hstu_attn_fwd_kv_rab_func_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                                    int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                                    int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                                    const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                                    int64_t head_dim, int64_t max_seqlen_q, int64_t max_seqlen_k, const int32_t* num_contexts,
                                    const int32_t* num_targets, int64_t target_group_size, int64_t window_left,
                                    int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                                    int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, const int32_t* func,
                                    int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                                    const void* kv_cache, const int32_t* page_offsets, const int32_t* page_ids,
                                    const int32_t* last_page_lens, int64_t page_size, hipStream_t stream);
/* The backward of the self-attention call: the recomputing passes (the key-major dV / dK pass(es) under the per-key-block table of
 * func_workspace, the query-major dQ pass under the func extents of its rows).  drab (nullable) as in mi355_hstu_attn_bwd_rab: one
 * [max_seqlen][max_seqlen] matrix per head, zero-filled by the caller; it receives dS wherever the row sees the key and zero where
 * the functions mask.  func_workspace / func_workspace_bytes as in mi355_hstu_attn_bwd_func (nullable). */
int mi355_hstu_attn_bwd_rab_func(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                                 int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                                 int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                                 const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                                 const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                                 int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                                 int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, void* drab,
                                 int64_t drab_batch_stride, int64_t drab_head_stride, int64_t drab_row_stride, const int32_t* func,
                                 int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                                 void* func_workspace, int64_t func_workspace_bytes, hipStream_t stream);
int mi355_hstu_attn_bwd_rab_func_f16(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                                 int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                                 int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                                 const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                                 const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                                 int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                                 int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, void* drab,
                                 int64_t drab_batch_stride, int64_t drab_head_stride, int64_t drab_row_stride, const int32_t* func,
                                 int64_t func_head_stride, int64_t func_bound_stride, int64_t n_func, float func_neg,
                                 void* func_workspace, int64_t func_workspace_bytes, hipStream_t stream);

/* append_kvcache (torch.ops.paged_kvcache_ops.append_kvcache, examples/commons/ops/cuda_ops/csrc/
 * paged_kvcache_ops_kernel.cu:106-140, call site paged_hstu_infer_layer.py:350-364): new-history token i (i < *nnz_dev,
 * or < max_nnz when max_nnz > 0) of sequence batch_indices[i] is written at position positions[i] of that user's
 * cache (page kv_indices[kv_indptr[batch] + pos / page_size], slot pos % page_size; NHD layout); its source row in
 * append_key / append_value is i + seqlen_offsets[batch].  nnz_upper bounds the launch when the count is on the device. */
int mi355_append_kvcache(void* kv_cache, const int32_t* kv_indices, const int32_t* kv_indptr, int64_t num_heads,
                         int64_t head_dim, int64_t page_size, const void* append_key, const void* append_value,
                         int64_t k_row_stride, int64_t v_row_stride, int64_t k_head_stride, int64_t v_head_stride,
                         const int32_t* batch_indices, const int32_t* positions, const int32_t* seqlen_offsets,
                         const int32_t* nnz_dev, int64_t max_nnz, int64_t nnz_upper, hipStream_t stream);

/* KV cache GPU tier (csrc/kvcache_ops.hip; 16-bit type-agnostic like mi355_append_kvcache).
 *
 * mi355_kvcache_move_pages: the page mover of the cache [L, P, 2, page_size, H, D], both directions, every layer of a range in
 * one launch (gather_kvcache and GatherPagedKVCacheAllLayers, examples/commons/ops/cuda_ops/csrc/paged_kvcache_ops_kernel.cu:
 * 237-429 and paged_kvcache_ops_cuda.cpp:229-321; the gather / scatter kernels of corelib/recsys_kvcache_manager/src/
 * gather_scatter_kernels.cu).  direction 0 (gather, offload): staging slot j of layer l becomes a bit-exact copy of page
 * page_ids[j] of layer l; direction 1 (scatter, onboard): the inverse.  A page is page_elems = 2 * page_size * H * D contiguous
 * elements in either kv_layout, so the mover is layout-agnostic.  cache points at the first layer of the range; the strides
 * between pages and between layers are given in elements for cache and staging separately and must be multiples of 8, both
 * pointers 16-byte aligned.  All offsets are 64 bits wide.  page_ids is int32 on the device, num_pages comes from the host: no
 * sync, no allocation, graph-capturable; num_pages == 0 returns without a launch.  A slot whose id is outside
 * [0, num_cache_pages) is skipped -- nothing is read or written, on a gather its staging slot keeps what it held.  Duplicate
 * ids in a scatter: which copy wins is undefined; in a gather they are fine.  grid_cap (256-thread blocks) and nontemporal (1:
 * nontemporal loads and stores, 0: plain) are measurement knobs: 0 and -1 select the measured defaults
 * (profiles/kvcache_pages_bench.txt).
 *
 * mi355_kvcache_batch_positions: the append metadata of a batch (GetPagedBatchIndicesPositions, paged_kvcache_ops_kernel.cu:
 * 451-492, called from gpu_kvcache_manager_impl.cpp:379-386).  Token i of sequence b (new_history_offsets[b] <= i <
 * new_history_offsets[b + 1]) gets batch_indices[i] = b and positions[i] = total_history_lengths[b] - (new_history_offsets[b + 1]
 * - new_history_offsets[b]) + (i - new_history_offsets[b]).  One thread per token; nnz = new_history_offsets[batch] comes from
 * the host. */
int mi355_kvcache_move_pages(int direction, void* cache, void* staging, const int32_t* page_ids, int64_t num_pages,
                             int64_t num_cache_pages, int64_t num_layers, int64_t page_elems, int64_t cache_page_stride,
                             int64_t cache_layer_stride, int64_t staging_page_stride, int64_t staging_layer_stride,
                             int64_t grid_cap, int nontemporal, hipStream_t stream);
int mi355_kvcache_batch_positions(const int32_t* new_history_offsets, const int32_t* total_history_lengths, int64_t batch,
                                  int64_t nnz, int32_t* batch_indices, int32_t* positions, hipStream_t stream);

/* hstu_varlen_bwd (hstu_api.cpp:525-719; hstu_varlen_bwd_80, fused_hstu_op.py:682-706): dq, dk, dv
 * contiguous bf16 [total, H, d].  Deterministic (two passes, no atomics): `deterministic` of the
 * reference is always on. */
int64_t mi355_hstu_attn_bwd_workspace_bytes(int64_t total_tokens, int64_t num_heads, int64_t head_dim);
/* Local (sliding window) attention: window_size = (left, right) of hstu_attn_varlen_func (hstu_attn_interface.py:196-222,
 * hstu_api.cpp:154-165): query i sees keys i - left .. i + right, a negative side is unbounded ((-1, 0) = causal,
 * (-1, -1) = full).  No contextual / target rows with a window; self attention only. */
int mi355_hstu_attn_fwd_window(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                               int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                               int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens,
                               int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen, int64_t window_left,
                               int64_t window_right, float alpha, float scaling_seqlen, hipStream_t stream);
int mi355_hstu_attn_bwd_window(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                               int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                               int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                               const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim,
                               int64_t max_seqlen, int64_t window_left, int64_t window_right, float alpha,
                               float scaling_seqlen, void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* Relative attention bias: `rab` / `has_drab` of hstu_attn_varlen_func (hstu_attn_interface.py:185-279; varlen_fwd /
 * varlen_bwd hstu_api.cpp:100-111,253-263,417-430,659-667).  rab: bf16 [batch][heads or 1][max_seqlen][max_seqlen] by its
 * batch / head / row strides in elements (head stride 0: one matrix for all heads), added to q_i . k_j before alpha and
 * SiLU.  Mask as window_size of hstu_attn_varlen_func: (-1, 0) causal (num_contexts / num_targets allowed), (-1, -1) full,
 * otherwise a local window.  Self attention over contiguous keys.  drab (nullable): bf16, one matrix per head with its own
 * strides, zero-filled by the caller; receives d loss / d rab at every position inside the sequences. */
int mi355_hstu_attn_fwd_rab(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride, int64_t k_row_stride,
                            int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride, int64_t k_head_stride,
                            int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens, int64_t batch,
                            int64_t num_heads, int64_t head_dim, int64_t max_seqlen, const int32_t* num_contexts,
                            const int32_t* num_targets, int64_t target_group_size, int64_t window_left, int64_t window_right,
                            float alpha, float scaling_seqlen, const void* rab, int64_t rab_batch_stride,
                            int64_t rab_head_stride, int64_t rab_row_stride, hipStream_t stream);
int mi355_hstu_attn_bwd_rab(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                            int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                            int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                            const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                            const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                            int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                            int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, void* drab,
                            int64_t drab_batch_stride, int64_t drab_head_stride, int64_t drab_row_stride, hipStream_t stream);
/* Delta-q backward: gradients of mi355_hstu_attn_fwd_kv / _kv_window / _kv_rab without a paged cache (hstu_bwd.h:98:
 * actual_seqlen_offset = actual_seqlen_k - actual_seqlen_q shifts every tile bound and mask of the reference's backward, :102-123,
 * 191-198,565-616; its kernel tests differentiate such calls, corelib/hstu/test.py:667-720).  The queries of sequence b (rows
 * cu_seqlens_q[b] .. of q / dout / dq) are the LAST Lq of its Lk keys (rows cu_seqlens_k[b] .. of k / v / dk / dv): query r sits
 * at the absolute position Lk - Lq + r, where the masks and rab[b][h][Lk - Lq + r][j] are taken.  Mask as window_size: (-1, 0)
 * causal (num_contexts / num_targets allowed), (-1, -1) full, otherwise a local window.  rab (nullable) as for
 * mi355_hstu_attn_fwd_kv_rab; drab (nullable, needs rab): one [max_seqlen_k][max_seqlen_k] matrix per head, zero-filled by the
 * caller -- rows in front of a sequence's first query and everything outside the sequence stay zero.  dq contiguous
 * [total_q, H, d], dk / dv contiguous [total_k, H, d]; every row is written (a sequence without queries, keys no query reaches:
 * zeros).  Deterministic, no scratch: the recomputing passes, their query / key tile loops clipped to what the shifted mask
 * reaches.  max_seqlen_q > max_seqlen_k is refused (MI355_EINVAL); Lq > Lk in a single sequence is visible on the device only
 * and undefined, as in the forward -- the passes then touch nothing of that sequence and its gradient rows stay unwritten. */
int mi355_hstu_attn_bwd_kv(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                           int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                           int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                           const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                           int64_t head_dim, int64_t max_seqlen_q, int64_t max_seqlen_k, const int32_t* num_contexts,
                           const int32_t* num_targets, int64_t target_group_size, int64_t window_left, int64_t window_right,
                           float alpha, float scaling_seqlen, const void* rab, int64_t rab_batch_stride,
                           int64_t rab_head_stride, int64_t rab_row_stride, void* drab, int64_t drab_batch_stride,
                           int64_t drab_head_stride, int64_t drab_row_stride, hipStream_t stream);
/* Optional scratch of mi355_hstu_attn_bwd: given a 16-byte aligned workspace of at least this many bytes, the dK pass
 * hands dS to the dQ pass through it (bf16, B * H * ceil(max_seqlen/32)^2 sub-tiles of 2 KB) and the dQ pass skips the
 * S / dP recomputation (head_dim >= 128: P travels too and the dV pass becomes one GEMM); with a smaller (or no)
 * workspace the passes recompute.  0: exchange switched off.
 * Results are bit-identical either way (the dQ GEMM consumes the same bf16 dS). */
int64_t mi355_hstu_attn_bwd_ds_bytes(int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen);
/* The same exchange under a byte cap: the workspace holds one chunk of (sequence, head) units at a time, each with the
 * ceil(L_b / 32)^2 tiles of its own length (scratch by the jagged sum, not B x max_seqlen^2), and mi355_hstu_attn_bwd walks
 * the chunks -- the reference's backward needs O(T) memory (hstu_bwd.h:687-729: dQ by atomics, no score-sized buffer); this
 * keeps the one-GEMM dV / dQ passes of the exchange with a bounded buffer.  Returns the workspace bytes to allocate
 * (<= cap_bytes, 256-byte aligned base required; 0 = no exchange fits, the recomputing passes run).  total_tokens: rows of q;
 * plain_causal: causal mask without contextual rows, window or bias -- the sub-tiles above the diagonal are then not stored. */
int64_t mi355_hstu_attn_bwd_ds_bytes_capped(int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                                            int64_t total_tokens, int64_t cap_bytes, int plain_causal);
/* total tokens of the NEXT mi355_hstu_attn_bwd call on this thread (its signature is the reference's hstu_varlen_bwd and
 * does not carry them): bounds the number of chunk passes; optional. */
void mi355_hstu_attn_bwd_hint_tokens(int64_t total_tokens);
/* row and head strides, in elements, of dq, dk, dv of the NEXT backward call on this thread: any of mi355_hstu_attn_bwd,
 * _bwd_window, _bwd_rab, _bwd_func, _bwd_kv and their _f16 twins (one binding for both operand types), whose signatures are the
 * reference's and take the three gradients as contiguous [total, H, d].  The callers this serves hand the kernel views into one
 * buffer: the fused layer's duvqk split (examples/hstu/ops/fused_hstu_op.py:932-1006, row stride (2 dl + 2 da) H) and the packed
 * dqkv[:, i] of hstu_attn_qkvpacked_func (corelib/hstu/hstu_attn/hstu_attn_interface.py:378-388, row stride 3 H d).  The gradients
 * are stored at base + row * row_stride + head * head_stride, the last dimension contiguous; rows that receive zeros (keys no
 * query reaches, a sequence without queries) receive them there.  That call takes the binding on entry: it is gone whether the
 * call succeeds, returns early (batch == 0) or fails an argument check.  Checked by that call, MI355_EINVAL otherwise: every
 * stride a multiple of 8 elements below 2^31, head strides >= head_dim.  Nothing bound: H d and d. */
void mi355_hstu_attn_bwd_bind_grad_strides(int64_t dq_row_stride, int64_t dq_head_stride, int64_t dk_row_stride,
                                           int64_t dk_head_stride, int64_t dv_row_stride, int64_t dv_head_stride);
/* rows of q of the NEXT mi355_hstu_attn_fwd / _fwd_kv / _fwd_window call on this thread (optional): batch x max_seqlen rows
 * = a dense batch, which the head-dim-256 forward runs with two row blocks (the z-th heaviest and z-th lightest of a column)
 * per workgroup.  The fp16 entry points have their own hint (suffix _f16). */
void mi355_hstu_attn_fwd_hint_tokens(int64_t total_tokens);
void mi355_hstu_attn_fwd_hint_tokens_f16(int64_t total_tokens);
int mi355_hstu_attn_bwd(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                        int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                        int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride,
                        int64_t do_head_stride, const int32_t* cu_seqlens, int64_t batch, int64_t num_heads,
                        int64_t head_dim, int64_t max_seqlen, const int32_t* num_contexts,
                        const int32_t* num_targets, int64_t target_group_size, int causal, float alpha,
                        float scaling_seqlen, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* fp16 operands (hstu_api.cpp:359-366: "HSTU only supports fp16 and bf16"): the same seven entry points for q / k / v / out /
 * gradients (and rab) in IEEE half instead of bf16 -- same kernels compiled with v_mfma_f32_32x32x16_f16, fp32
 * accumulation, round-to-nearest-even packing.  The size queries and append_kvcache are type-agnostic. */
int mi355_hstu_attn_fwd_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                        int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                        int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                        const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim,
                        int64_t max_seqlen, const int32_t* num_contexts, const int32_t* num_targets,
                        int64_t target_group_size, int causal, float alpha, float scaling_seqlen,
                        hipStream_t stream);
int mi355_hstu_attn_fwd_kv_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                           int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                           int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride,
                           const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                           int64_t head_dim, int64_t max_seqlen_q, const int32_t* num_contexts,
                           const int32_t* num_targets, int64_t target_group_size, int causal, float alpha,
                           float scaling_seqlen, const void* kv_cache, const int32_t* page_offsets,
                           const int32_t* page_ids, const int32_t* last_page_lens, int64_t page_size,
                           hipStream_t stream);
int mi355_hstu_attn_bwd_f16(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                        int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                        int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride,
                        int64_t do_head_stride, const int32_t* cu_seqlens, int64_t batch, int64_t num_heads,
                        int64_t head_dim, int64_t max_seqlen, const int32_t* num_contexts,
                        const int32_t* num_targets, int64_t target_group_size, int causal, float alpha,
                        float scaling_seqlen, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int mi355_hstu_attn_fwd_window_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                               int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                               int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens,
                               int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen, int64_t window_left,
                               int64_t window_right, float alpha, float scaling_seqlen, hipStream_t stream);
int mi355_hstu_attn_bwd_window_f16(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                               int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                               int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                               const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim,
                               int64_t max_seqlen, int64_t window_left, int64_t window_right, float alpha,
                               float scaling_seqlen, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int mi355_hstu_attn_fwd_rab_f16(const void* q, const void* k, const void* v, void* out, int64_t q_row_stride, int64_t k_row_stride,
                            int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride, int64_t k_head_stride,
                            int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens, int64_t batch,
                            int64_t num_heads, int64_t head_dim, int64_t max_seqlen, const int32_t* num_contexts,
                            const int32_t* num_targets, int64_t target_group_size, int64_t window_left, int64_t window_right,
                            float alpha, float scaling_seqlen, const void* rab, int64_t rab_batch_stride,
                            int64_t rab_head_stride, int64_t rab_row_stride, hipStream_t stream);
int mi355_hstu_attn_bwd_rab_f16(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                            int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                            int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                            const int32_t* cu_seqlens, int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                            const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                            int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen, const void* rab,
                            int64_t rab_batch_stride, int64_t rab_head_stride, int64_t rab_row_stride, void* drab,
                            int64_t drab_batch_stride, int64_t drab_head_stride, int64_t drab_row_stride, hipStream_t stream);
int mi355_hstu_attn_bwd_kv_f16(const void* dout, const void* q, const void* k, const void* v, void* dq, void* dk, void* dv,
                           int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t do_row_stride,
                           int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride, int64_t do_head_stride,
                           const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k, int64_t batch, int64_t num_heads,
                           int64_t head_dim, int64_t max_seqlen_q, int64_t max_seqlen_k, const int32_t* num_contexts,
                           const int32_t* num_targets, int64_t target_group_size, int64_t window_left, int64_t window_right,
                           float alpha, float scaling_seqlen, const void* rab, int64_t rab_batch_stride,
                           int64_t rab_head_stride, int64_t rab_row_stride, void* drab, int64_t drab_batch_stride,
                           int64_t drab_head_stride, int64_t drab_row_stride, hipStream_t stream);


/* ---- HSTU attention on FP8 (OCP e4m3fn) operands (csrc/hstu_fp8.hip) ----
 * Quantisers of hopper/hstu_attn_interface.py:32-292 (quantize_for_two_directions, quantize_for_block_scale,
 * quantize_for_head_batch_tensor), bit for bit: x [total, num_heads, head_dim] bf16 (x_is_f16 = 0) or fp16, contiguous;
 * out_fp8 the same shape in e4m3fn bytes.  kind:
 *   0  x.to(float8_e4m3fn) (quant_mode 0; no descale)
 *   1  per (token, head) (quant_mode 1, q / k: :40-49): descale[h * descale_stride + t]
 *   2  per (128-token tile, head, column) (quant_mode 1, vt: :51-117): descale [num tiles, num_heads, head_dim]
 *   3  per (block_size-token tile, head) (quant_mode 2: :119-192): descale[h * descale_stride + tile]
 *   4 / 5 / 6  per (sequence, head) / sequence / tensor (quant_mode 3 / 4 / 5: :223-292): descale [B, H] / [B] / [1]
 * Kinds 2 .. 6 walk the tiles of cu_blocks (mi355_hstu_fp8_cu_blocks with block_size 128, or the mode-2 block size);
 * num_blocks_bound >= its last entry sizes the grid (mi355_hstu_fp8_blocks_bound).  Kinds 4 .. 6 take amax_work, a zeroed
 * uint32 array of one entry per descale. */
int mi355_hstu_fp8_cu_blocks(const int32_t* seq_offsets, int64_t batch, int64_t block_size, int32_t* cu_blocks,
                             hipStream_t stream);
int64_t mi355_hstu_fp8_blocks_bound(int64_t total, int64_t batch, int64_t block_size);
int mi355_hstu_fp8_quantize(int kind, const void* x, int x_is_f16, int64_t total, int64_t num_heads, int64_t head_dim,
                            const int32_t* seq_offsets, int64_t batch, int64_t block_size, const int32_t* cu_blocks,
                            int64_t num_blocks_bound, void* out_fp8, float* descale, int64_t descale_stride,
                            uint32_t* amax_work, hipStream_t stream);
/* FP8 forward of self-attention (cu_seqlens_q == cu_seqlens_k): the quant_mode 0 .. 5 arms of hstu_hopper_cuda.varlen_fwd
 * (hopper/hstu_api.cpp:520-566; arithmetic mainloop_fwd_sm90_tma_gmma_ws.hpp:1342-1470).  q / k / v: e4m3fn bytes with
 * row / head strides in bytes (multiples of 16); in mode 1, v is the reference's vt.  out: fp16, strides in elements.
 * head_dim 64 / 128 / 256; masks as mi355_hstu_attn_fwd_rab (window_left / window_right, num_contexts / num_targets with the
 * causal window (-1, 0)).  Descales per mode: 1: descale_q / descale_k [H, >= total] (row stride = descale_*_stride),
 * descale_v = descale_vt [tiles, H, head_dim] (tile stride = descale_v_stride) with cu_seqlens_descale_vt;
 * 2: [H, blocks] with cu_seqlens_block_descale_q (128-row blocks) / _kv (block_kv = 64 or 128 keys); 3: [B, H]; 4: [B];
 * 5: [1]; mode 0 reads none. */
int mi355_hstu_attn_fwd_fp8(int quant_mode, const void* q, const void* k, const void* v, void* out, int64_t q_row_stride,
                            int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride, int64_t q_head_stride,
                            int64_t k_head_stride, int64_t v_head_stride, int64_t o_head_stride, const int32_t* cu_seqlens,
                            int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                            const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                            int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen,
                            const float* descale_q, const float* descale_k, const float* descale_v,
                            int64_t descale_q_stride, int64_t descale_k_stride, int64_t descale_v_stride,
                            const int32_t* cu_seqlens_descale_vt, const int32_t* cu_seqlens_block_descale_q,
                            const int32_t* cu_seqlens_block_descale_kv, int64_t block_kv, hipStream_t stream);

/* FP8 backward of self-attention: the quant_mode 0 .. 5 arms of hstu_hopper_cuda.varlen_bwd (hopper/hstu_api.cpp:809-1010;
 * arithmetic mainloop_bwd_sm90_tma_gmma_ws.hpp:1496-2342).  dout / dout_t / q / q_t / k / k_t / v: e4m3fn bytes; dout_t,
 * q_t, k_t are read in mode 1 only (the reference's transposed-direction quantisations, token-major here) and may be null
 * otherwise.  dq / dk / dv: fp16 outputs.  row_strides[10] / head_strides[10] (host arrays) in the order dout, dout_t, q,
 * q_t, k, k_t, v (bytes, multiples of 16), dq, dk, dv (elements, multiples of 4).  Masks, alpha and scaling_seqlen as
 * mi355_hstu_attn_fwd_fp8.  Descales per mode (descale_strides[7], host, in the order q, qt, k, kt, v, do, dot):
 * 1: descale_q / _k / _v / _do [H, >= total] (row stride), descale_qt / _kt / _dot [tiles, H, head_dim] (tile stride) with
 * cu_seqlens_descale_qt (qt, dot) / _kt (kt); 2: [H, blocks] with cu_seqlens_block_descale_q (64-token q / dout blocks) and
 * _kv (128-token k / v blocks); 3: [B, H]; 4: [B]; 5: [1]; mode 0 reads none.  Deterministic: no atomics, no workspace. */
int mi355_hstu_attn_bwd_fp8(int quant_mode, const void* dout, const void* dout_t, const void* q, const void* q_t,
                            const void* k, const void* k_t, const void* v, void* dq, void* dk, void* dv,
                            const int64_t* row_strides, const int64_t* head_strides, const int32_t* cu_seqlens,
                            int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                            const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                            int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen,
                            const float* descale_q, const float* descale_qt, const float* descale_k,
                            const float* descale_kt, const float* descale_v, const float* descale_do,
                            const float* descale_dot, const int64_t* descale_strides,
                            const int32_t* cu_seqlens_descale_qt, const int32_t* cu_seqlens_descale_kt,
                            const int32_t* cu_seqlens_block_descale_q, const int32_t* cu_seqlens_block_descale_kv,
                            hipStream_t stream);

/* ---- hstu_cuda_ops: jagged row movers between the embedding output and the attention input (csrc/jagged_ops.hip) ----
 * Reference paths below are relative to the reference's examples/commons/ops/cuda_ops/.  dtype codes as everywhere
 * (0 fp32, 1 bf16, 2 fp16) plus 3 = fp64 for these entry points: rows are moved as bytes. */

/* Concat of n (1..128) jagged 2-D tensors with one hidden dim D and one batch, and its inverse: replaces
 * concat_2D_jagged_tensors_cuda_forward / _backward (csrc/jagged_tensor_op_kernel.cu; op schema
 * csrc/jagged_tensor_op_cuda.cpp:243-244).  values / offsets / rows are HOST arrays of n entries (device pointer of tensor t,
 * device pointer of its int64 offsets [batch + 1], its row count); they travel to the kernel as arguments, nothing is staged.
 * direction 0: merged[merged_offsets[b] + sum_{t' < t} len_t'[b] + r, :] = values_t[offsets_t[b] + r, :];
 * direction 1: the inverse, every row of every values_t is written.  merged: [total_rows, D].  One launch, no host sync, no
 * allocation; a row index outside its tensor (inconsistent offsets) is skipped, never accessed. */
int mi355_jagged_concat(int n, const void* const* values, const int64_t* const* offsets, const int64_t* rows, int64_t batch,
                        const int64_t* merged_offsets, void* merged, int64_t total_rows, int64_t D, int dtype,
                        int direction, hipStream_t stream);

/* compute_block_workloads (csrc/jagged_tensor_op_kernel.cu; schema csrc/jagged_tensor_op_cuda.cpp:245): with
 * nb = ceil(max_seqlen / seqlen_per_block), workloads[(b n + t) nb + idx] = max(0, min(len_t[b] - idx seqlen_per_block,
 * seqlen_per_block)).  offsets: HOST array of n device pointers.  Only the reference's Python wrapper needs it. */
int mi355_jagged_block_workloads(int n, const int64_t* const* offsets, int64_t batch, int64_t seqlen_per_block,
                                 int64_t max_seqlen, int64_t* workloads, int64_t workloads_numel, hipStream_t stream);

/* Row movement of hstu_inference_preprocess (csrc/jagged_tensor_op_cuda.cpp:135-240, a host loop of narrow().copy_() there) in
 * one launch.  Per sample with I items, A actions (e = A - I in {0, 1}) and C candidates, h = I - C: output row r is
 * action[0] if r < e; with r' = r - e: item[r' / 2] (r' < 2 h, even), action[r' / 2 + e] (r' < 2 h, odd), else
 * item[h + r' - 2 h]; the candidates' action rows are dropped.  All offsets are device int64 [batch + 1]; C follows from
 * them (out length = 2 h + e + C). */
int mi355_hstu_inference_preprocess(const void* item_values, int64_t item_rows, const int64_t* item_offsets,
                                    const void* action_values, int64_t action_rows, const int64_t* action_offsets,
                                    const int64_t* out_offsets, int64_t batch, void* out, int64_t out_rows, int64_t D,
                                    int dtype, hipStream_t stream);

/* ---- HSTU positional encoder (csrc/position_ops.hip) ----
 * Reference paths below are examples/hstu/ops/triton_ops/triton_position.py, Triton kernels there.  All row strides are in
 * ELEMENTS (>= D, last dimension contiguous); D is any positive value.  offsets [batch + 1], lengths, high_inds, ind_offsets,
 * num_targets [batch] and timestamps [rows] are device int64.  A table is fp32 or has the dtype of the rows.  No host sync, no
 * allocation, capturable; rows outside every sequence [offsets[b], offsets[b + 1]) are neither read nor written. */

/* _add_position_embeddings_kernel (:80-137).  For row n of sequence b, i = n + (ind_offsets ? ind_offsets[b] : 0),
 * idx = i >= high_inds[b] ? high_inds[b] : i, out = round(jagged * scale + dense[idx]) with one fp32 fused multiply-add.
 * UNLIKE the reference, idx is then clamped into [0, K - 1]: nothing outside dense [K, D] is ever accessed. */
int mi355_hstu_add_position_embeddings(const void* jagged, int64_t jagged_stride, int64_t rows, int64_t D, int dtype,
                                       const int64_t* offsets, const int64_t* high_inds, const int64_t* ind_offsets,
                                       int64_t batch, const void* dense, int64_t dense_stride, int64_t K, int dense_dtype,
                                       float scale, void* out, int64_t out_stride, hipStream_t stream);

/* _add_position_embeddings_bwd_kernel (:141-211), the case without ind_offsets (:268-270).  d_jagged = round(d_out * scale) when
 * d_jagged is non-null (the caller passes null for scale == 1 and returns d_out).  d_dense[k] = the sum of the d_out rows whose
 * idx is k, accumulated in fp32 in a fixed order (bitwise reproducible, no atomics) and rounded once to dense_dtype (the
 * reference rounds to the dtype of d_out first); all K rows are written, a row nothing maps to as zeros.  workspace: 32-byte
 * aligned, mi355_hstu_add_position_embeddings_bwd_workspace_bytes(rows, batch, D) bytes, contents irrelevant. */
int64_t mi355_hstu_add_position_embeddings_bwd_workspace_bytes(int64_t rows, int64_t batch, int64_t D);
int mi355_hstu_add_position_embeddings_bwd(const void* d_out, int64_t d_out_stride, int64_t rows, int64_t D, int dtype,
                                           const int64_t* offsets, const int64_t* high_inds, int64_t batch, float scale,
                                           void* d_jagged, int64_t d_jagged_stride, void* d_dense, int64_t d_dense_stride,
                                           int64_t K, int dense_dtype, void* workspace, int64_t workspace_bytes,
                                           hipStream_t stream);

/* _add_timestamp_position_embeddings_kernel (:309-404).  Row n of sequence b [s, e):
 *   high = lengths[b] - (num_targets ? (interleave_targets ? 2 : 1) * num_targets[b] : 0);
 *   p = high - min(n, high) + max_contextual_seq_len; p = min(p, Np - 1); if n < max_contextual_seq_len: p = n;
 *   dt = max(float(timestamps[e - 1] - timestamps[s + n] + time_delta), 1e-6f) / time_bucket_increments (IEEE division);
 *   t = int32(f(dt) * time_bucket_scale), f = sqrtf (time_bucket_fn 0, correctly rounded) or logf (1), clamped into
 *   [0, num_time_buckets];  out = round(seq + round(pos_emb[p] + ts_emb[t])), both sums in fp32 (:399).
 * UNLIKE the reference, p is clamped into [0, Np - 1] and t into [0, Nt - 1] before the loads.  pos_inds / ts_inds (int32
 * [rows], may be null) receive p and t of every row. */
int mi355_hstu_add_timestamp_position_embeddings(const void* seq, int64_t seq_stride, int64_t rows, int64_t D, int dtype,
                                                 const int64_t* offsets, const int64_t* lengths, int64_t batch,
                                                 const void* pos_emb, int64_t pos_stride, int64_t Np, const void* ts_emb,
                                                 int64_t ts_stride, int64_t Nt, int table_dtype, const int64_t* timestamps,
                                                 const int64_t* num_targets, int interleave_targets,
                                                 int64_t max_contextual_seq_len, int time_bucket_fn, int64_t num_time_buckets,
                                                 float time_bucket_increments, float time_bucket_scale, int64_t time_delta,
                                                 void* out, int64_t out_stride, int32_t* pos_inds, int32_t* ts_inds,
                                                 hipStream_t stream);

/* _add_embeddings_bwd_kernel (:434-482, float atomics there).  d_table[k] = the sum of d_out[sorted_rows[i]] over the i with
 * sorted_keys[i] == k: sorted_keys (int32 [count]) ascending, sorted_rows (int64 [count]) the d_out row of each entry (a stable
 * sort of the forward's pos_inds / ts_inds).  fp32 accumulation in list order per chunk of 64 or 32 entries, chunks in order: bitwise
 * reproducible, no atomics; all K rows written in table_dtype; keys outside [0, K) and rows outside [0, rows) are skipped.
 * workspace: 32-byte aligned, mi355_hstu_index_rows_sum_workspace_bytes(count, K, D) bytes. */
int64_t mi355_hstu_index_rows_sum_workspace_bytes(int64_t count, int64_t K, int64_t D);
int mi355_hstu_index_rows_sum(const void* d_out, int64_t d_out_stride, int64_t rows, int64_t D, int dtype,
                              const int32_t* sorted_keys, const int64_t* sorted_rows, int64_t count, void* d_table,
                              int64_t table_stride, int64_t K, int table_dtype, void* workspace, int64_t workspace_bytes,
                              hipStream_t stream);

/* ---- HSTU layer norms (csrc/norm_ops.hip) ----
 * Reference paths below are examples/hstu/ops/triton_ops/, Triton kernels there.  Rows are [rows, D], D in 1 .. 8192, last
 * dimension contiguous; every row tensor has its own row stride in ELEMENTS.  Rows are fp32 / bf16 / fp16 (`dtype`); weight and
 * bias [D] are contiguous, fp32 or of the row dtype (`weight_dtype`); mean and rstd are fp32 [rows].  All arithmetic is fp32 and
 * every stored value is rounded once.  No host sync, no allocation, capturable.  Determinism: no atomics; dweight / dbias are
 * fp32 sums over the rows in an order fixed by (rows, D), so every output is bitwise reproducible from call to call.
 *
 * Dropout (ln_mul_dropout): NOT Triton's tl.rand stream.  Element (row, col) of mask `which` (0 / 1 / 2 for the u / x / t
 * part of a concat_ux output, 0 otherwise) draws r = word (col & 3) of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32)
 * and counter (row & 0xffffffff, row >> 32, col >> 2, which); it is kept iff r >= floor(dropout_ratio * 2^32) (unsigned), a
 * kept value is v / (1.0f - (float)dropout_ratio), a dropped one +0.  training == 0 or dropout_ratio == 0: nothing dropped.
 * The mask is a function of (seed, row, col, which, dropout_ratio) alone, never of the launch geometry. */

/* _layer_norm_fwd / _weighted_layer_norm_fwd (triton_layer_norm.py:313-383).  mean = sum(x) / D, var = sum((x - mean)^2) / D
 * from the row held on chip, rstd = 1 / sqrt(var + eps), y = (x - mean) rstd w + b; weight == bias == null: w = 1, b = 0.
 * stats_given != 0: mean / rstd are read as given and nothing is recomputed (COMPUTE_MEAN_AND_RSTD false there); else written. */
int mi355_hstu_layer_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                              const void* bias, int weight_dtype, float eps, void* y, int64_t y_stride, float* mean, float* rstd,
                              int stats_given, hipStream_t stream);

/* _layer_norm_bwd_dx / _weighted_layer_norm_bwd_dx + _layer_norm_bwd_dwdb (triton_layer_norm.py:386-481).  xh = (x - mean) rstd,
 * g = w dy, c1 = sum(xh g) / D, c2 = sum(g) / D, dx = (g - (xh c1 + c2)) rstd + dx_accumulate (may be null; added in fp32 before
 * the rounding).  weight non-null: dweight = sum_rows dy xh, dbias = sum_rows dy in weight_dtype (zeros for rows == 0), and
 * workspace (16-byte aligned, mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D), contents irrelevant) is needed. */
int64_t mi355_hstu_layer_norm_bwd_workspace_bytes(int64_t rows, int64_t D);
int mi355_hstu_layer_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D,
                              int dtype, const void* weight, int weight_dtype, const float* mean, const float* rstd,
                              const void* dx_accumulate, int64_t dx_accumulate_stride, void* dx, int64_t dx_stride, void* dweight,
                              void* dbias, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* _ln_mul_dropout_fwd (triton_norm_mul_dropout.py:36-127, :361-423).  ln as above, t = ln u; y [rows, D] = drop(t), or with
 * concat_ux y [rows, 3 D] = [drop0(u) | drop1(x) | drop2(t)].  u is [rows, H, UD] with strides (u_stride0, u_stride1, 1) and
 * H UD == D (a 2-D u: H = 1, UD = D).  Writes mean and rstd. */
int mi355_hstu_ln_mul_dropout_fwd(const void* x, int64_t x_stride, const void* u, int64_t u_stride0, int64_t u_stride1, int64_t H,
                                  int64_t UD, int64_t rows, int64_t D, int dtype, const void* weight, const void* bias,
                                  int weight_dtype, float eps, double dropout_ratio, int training, uint64_t seed, int concat_ux,
                                  void* y, int64_t y_stride, float* mean, float* rstd, hipStream_t stream);

/* _ln_mul_dropout_bwd_dx_du + _ln_mul_dropout_bwd_dwdb (triton_norm_mul_dropout.py:130-358, :426-525).  The masks are made again
 * from the seed.  dy is [rows, D], or [rows, 3 D] = [dy_u | dy_x | dy_t] with concat_ux.  dt = drop2'(dy_t);
 * du = dt ln (+ drop0'(dy_u)), written with the strides of du (layout of u); dx = the layer-norm backward of g = w dt u
 * (+ drop1'(dy_x)); dweight = sum_rows dt u xh, dbias = sum_rows dt u.  y non-null: the forward's output is written again,
 * bit-equal to the forward's.  workspace as above, mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(rows, D). */
int64_t mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(int64_t rows, int64_t D);
int mi355_hstu_ln_mul_dropout_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* u,
                                  int64_t u_stride0, int64_t u_stride1, int64_t H, int64_t UD, int64_t rows, int64_t D, int dtype,
                                  const void* weight, const void* bias, int weight_dtype, const float* mean, const float* rstd,
                                  double dropout_ratio, int training, uint64_t seed, int concat_ux, void* dx, int64_t dx_stride,
                                  void* du, int64_t du_stride0, int64_t du_stride1, void* dweight, void* dbias, void* y,
                                  int64_t y_stride, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- HSTU norm family (csrc/group_norm_ops.hip, csrc/norm_family_ops.hip) ----
 * Group norm mul dropout, swish layer norm and RMS norm under the conventions of the layer norms above: fp32 arithmetic, every
 * stored value rounded once; rows fp32 / bf16 / fp16, weights fp32 or of the row dtype; a row stride in ELEMENTS per row tensor,
 * last dimension contiguous; row width 1 .. 8192; no host sync, no allocation, capturable; no atomics, every output bitwise
 * reproducible.  rows == 0 is a successful no-op; a backward with rows == 0 still writes zero parameter gradients (so dweight /
 * dbias are needed then, the workspace is not). */

/* _group_norm_mul_dropout_fwd (triton_norm_mul_dropout.py:601-686, :842-911; pt_ops/pt_norm_mul_dropout.py:38-45).  x is
 * [rows, H L] (D == H L), u [rows, H, L] with strides (u_stride0, u_stride1, 1) (a 2-D u: u_stride1 = L); weight and bias [H],
 * both required; mean and rstd fp32 [rows H] at row H + h.  Per (row, head): mean = sum(x) / L, var = sum((x - mean)^2) / L in
 * a second pass over the head, rstd = 1 / sqrtf(var + eps), xh = (x - mean) rstd, gn = fmaf(xh, w_h, b_h), t = gn u.
 * y [rows, H L] = drop(t), or with concat_ux y [rows, 3 H L] = [drop0(u) | drop1(x) | drop2(t)]; the dropout is the stream
 * defined above with col the column in the whole row, h L + c: with H == 1 the masks are those of
 * mi355_hstu_ln_mul_dropout_fwd for the same seed. */
int mi355_hstu_gn_mul_dropout_fwd(const void* x, int64_t x_stride, const void* u, int64_t u_stride0, int64_t u_stride1, int64_t H,
                                  int64_t L, int64_t rows, int64_t D, int dtype, const void* weight, const void* bias,
                                  int weight_dtype, float eps, double dropout_ratio, int training, uint64_t seed, int concat_ux,
                                  void* y, int64_t y_stride, float* mean, float* rstd, hipStream_t stream);

/* _group_norm_mul_dropout_bwd_dx_du + _group_norm_bwd_dwdb (triton_norm_mul_dropout.py:689-839, :914-1039).  The masks are made
 * again from the seed.  dy is [rows, D], or [rows, 3 D] = [dy_u | dy_x | dy_t] with concat_ux.  dt = drop2'(dy_t);
 * du = dt gn (+ drop0'(dy_u)), written with the strides of du (layout of u); per head g = w_h dt u, c1 = sum(xh g) / L,
 * c2 = sum(g) / L, dx = (g - (xh c1 + c2)) rstd (+ drop1'(dy_x)); dweight[h] = sum over rows and the head's columns of dt u xh,
 * dbias[h] likewise of dt u: fp32 sums in an order fixed by (rows, H, L) and the 16-byte alignment of the pointers and strides,
 * rounded once to weight_dtype.  y non-null: the forward's output is written again, bit-equal to the forward's.  workspace:
 * 16-byte aligned, mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(rows, H, L), contents irrelevant. */
int64_t mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(int64_t rows, int64_t H, int64_t L);
int mi355_hstu_gn_mul_dropout_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* u,
                                  int64_t u_stride0, int64_t u_stride1, int64_t H, int64_t L, int64_t rows, int64_t D, int dtype,
                                  const void* weight, const void* bias, int weight_dtype, const float* mean, const float* rstd,
                                  double dropout_ratio, int training, uint64_t seed, int concat_ux, void* dx, int64_t dx_stride,
                                  void* du, int64_t du_stride0, int64_t du_stride1, void* dweight, void* dbias, void* y,
                                  int64_t y_stride, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* SwishLayerNormFunction.forward (triton_layer_norm.py:763-816; the IS_SWISH branch of _weighted_layer_norm_fwd).  weight and
 * bias [D], both required.  mean, rstd, xh and ln = fmaf(xh, w, b) as in mi355_hstu_layer_norm_fwd; s = 1 / (1 + expf(-ln)),
 * evaluated as the sigmoid of mi355_hstu_silu_bwd; y = s x.  Writes mean and rstd. */
int mi355_hstu_swish_layer_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                                    const void* bias, int weight_dtype, float eps, void* y, int64_t y_stride, float* mean,
                                    float* rstd, hipStream_t stream);

/* SwishLayerNormFunction.backward (triton_layer_norm.py:818-877; the IS_SWISH branch of _weighted_layer_norm_bwd_dx, :229-253).
 * q = ((dy x) s) (1 - s), g = w q, c1 = sum(xh g) / D, c2 = sum(g) / D, dx = (g - (xh c1 + c2)) rstd + dy s;
 * dweight = sum_rows q xh, dbias = sum_rows q in weight_dtype.  workspace: 16-byte aligned,
 * mi355_hstu_swish_layer_norm_bwd_workspace_bytes(rows, D). */
int64_t mi355_hstu_swish_layer_norm_bwd_workspace_bytes(int64_t rows, int64_t D);
int mi355_hstu_swish_layer_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D,
                                    int dtype, const void* weight, const void* bias, int weight_dtype, const float* mean,
                                    const float* rstd, void* dx, int64_t dx_stride, void* dweight, void* dbias, void* workspace,
                                    int64_t workspace_bytes, hipStream_t stream);

/* _weighted_rms_norm_fwd (triton_layer_norm.py:537-568, :660-704).  weight [D], required; no bias, no mean.
 * rstd = 1 / sqrtf(sum(x^2) / D + eps), xh = x rstd, y = xh w.  Writes rstd. */
int mi355_hstu_rms_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                            int weight_dtype, float eps, void* y, int64_t y_stride, float* rstd, hipStream_t stream);

/* _weighted_rms_norm_bwd_dx + _rms_norm_bwd_dwdb (triton_layer_norm.py:571-657, :706-760).  xh = x rstd, g = w dy,
 * c1 = sum(xh g) / D, dx = (g - xh c1) rstd; dweight = sum_rows dy xh in weight_dtype.  workspace: 16-byte aligned,
 * mi355_hstu_rms_norm_bwd_workspace_bytes(rows, D). */
int64_t mi355_hstu_rms_norm_bwd_workspace_bytes(int64_t rows, int64_t D);
int mi355_hstu_rms_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype,
                            const void* weight, int weight_dtype, const float* rstd, void* dx, int64_t dx_stride, void* dweight,
                            void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- HSTU activations (csrc/act_ops.hip) ----
 * The two element-wise steps of the fused HSTU layer (examples/hstu/ops/fused_hstu_op.py) that lie between the GEMMs.  Rows are
 * [rows, N] in fp32 / bf16 / fp16 (`dtype`), last dimension contiguous, every pointer with its own row stride in ELEMENTS
 * (>= N when rows > 1).  All arithmetic is fp32 and every stored value is rounded once.  No host sync, no allocation,
 * capturable.  rows == 0 or N == 0 is a successful no-op (the backward still writes dbias = 0). */

/* triton_silu.py (_silu_forward) and the SILU epilogue of triton_addmm.py:_addmm_optional_silu_fwd:
 * s = z / (1 + expf(-z)).  s may be z (in place: same pointer and stride). */
int mi355_hstu_silu_fwd(const void* z, int64_t z_stride, int64_t rows, int64_t N, int dtype, void* s, int64_t s_stride,
                        hipStream_t stream);

/* triton_silu.py (_silu_backward), and with dbias the pair aten.silu_backward + torch.sum(dz, 0) of triton_addmm_silu_bwd
 * (triton_addmm.py:278-309) in one pass: sig = 1 / (1 + expf(-z)), dz = g sig (1 + z (1 - sig)); dz may be g (in place).
 * dbias non-null: dbias[c] = sum over rows of the fp32 dz[., c] BEFORE its rounding, in an order fixed by (rows, N) alone (no
 * atomics, bitwise reproducible, the same for every dtype and layout), rounded once to dbias_dtype (fp32 or `dtype`); this needs
 * workspace (16-byte aligned, mi355_hstu_silu_bwd_workspace_bytes(rows, N), contents irrelevant).  dbias null: no sums, no
 * workspace. */
int64_t mi355_hstu_silu_bwd_workspace_bytes(int64_t rows, int64_t N);
int mi355_hstu_silu_bwd(const void* g, int64_t g_stride, const void* z, int64_t z_stride, int64_t rows, int64_t N, int dtype,
                        void* dz, int64_t dz_stride, void* dbias, int dbias_dtype, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream);

/* ---- jagged x dense products (csrc/jagged_bmm.hip) ----
 * The jagged-dense ops of examples/commons/ops/triton_ops/triton_jagged.py.  A jagged tensor is [L, width] rows in fp32 / bf16 /
 * fp16 (`dtype`), last dimension contiguous, with a row stride in ELEMENTS (>= the width when L > 1); `offsets` is int64
 * [batch + 1] on the device, sample b owning the rows offsets[b] .. offsets[b + 1] - 1.  Offsets are clamped to [0, L]; rows at
 * or past offsets[batch] belong to no sample and are never read.  The grids are sized from L and batch alone: no host read of an
 * offset, no max_seq_len, no allocation, capturable.  All arithmetic is fp32, every stored value is rounded once; no atomics,
 * every output bitwise reproducible.  L == 0 is a successful no-op for the per-row outputs; the per-sample outputs are still
 * written (zeros). */

/* jagged_dense_bmm_broadcast_add_kernel (triton_jagged.py:77-153; its callers :258-363 and :540-648).
 * out[r, :N] = jagged[r, :K] . dense_b[K, N] (+ bias[b, :N]) for the rows r of sample b; dense_b[k, n] is read at
 * dense + b stride_db + k stride_dk + n stride_dn (elements), so the backward's d_jagged = d_out . dense_b^T is this entry point
 * with stride_dk and stride_dn swapped and bias null.  bias may be null; bias_stride is its row stride.  Rows of `out` at or
 * past offsets[batch] are written as zeros.  bf16 / fp16: v_mfma_f32_32x32x16; fp32: v_mfma_f32_32x32x2_f32 (an fmaf chain in k
 * order).  The bias is added to the fp32 sum before the rounding. */
int mi355_jagged_dense_bmm(const void* jagged, int64_t jagged_stride, const int64_t* offsets, int64_t batch, int64_t L, int64_t K,
                           int64_t N, const void* dense, int64_t stride_db, int64_t stride_dk, int64_t stride_dn,
                           const void* bias, int64_t bias_stride, void* out, int64_t out_stride, int dtype, hipStream_t stream);

/* _jagged_jagged_bmm_reduce_sum (triton_jagged.py:161-255).  out[b, :M, :N] = a_rows[rows of b, :M]^T . b_rows[rows of b, :N], at
 * out + b out_stride_b + m out_stride_m + n; col_sum non-null: col_sum[b, :N] = sum over the rows of b of b_rows (row stride
 * col_sum_stride), taken by the same MFMAs against a tile of ones, in the order of out.  These are d_dense and d_bias of
 * mi355_jagged_dense_bmm.  An empty sample writes zeros.  A sample is summed in row order in chunks of C rows counted from its
 * first row (C = 64 rows per 64 x 64 tile of out, within 256 .. 4096: a function of M and N); the chunk sums of a sample longer
 * than C go through `workspace` and are added in chunk order, so the order of all additions is a function of (length, M, N)
 * alone.  workspace: 16-byte aligned, mi355_jagged_jagged_bmm_workspace_bytes(batch, L, M, N), contents irrelevant. */
int64_t mi355_jagged_jagged_bmm_workspace_bytes(int64_t batch, int64_t L, int64_t M, int64_t N);
int mi355_jagged_jagged_bmm(const void* a_rows, int64_t a_stride, const void* b_rows, int64_t b_stride, const int64_t* offsets,
                            int64_t batch, int64_t L, int64_t M, int64_t N, void* out, int64_t out_stride_b, int64_t out_stride_m,
                            void* col_sum, int64_t col_sum_stride, int dtype, void* workspace, int64_t workspace_bytes,
                            hipStream_t stream);

/* jagged_dense_broadcast_add_kernel (triton_jagged.py:387-437).  out[r, :D] = jagged[r, :D] + dense[b, :D] for the rows r of
 * sample b: one fp32 add, one rounding.  Rows at or past offsets[batch] are written as zeros.  16-byte accesses where D, every
 * base pointer and every stride allow, else element by element (same values). */
int mi355_jagged_broadcast_add(const void* jagged, int64_t jagged_stride, const int64_t* offsets, int64_t batch, int64_t L,
                               int64_t D, const void* dense, int64_t dense_stride, void* out, int64_t out_stride, int dtype,
                               hipStream_t stream);

/* jagged_reduce_sum (triton_jagged.py:440-477).  out[b, :D] = sum over the rows of sample b (zeros for an empty one): fp32,
 * 16 interleaved runs in row order folded in run order (a function of the length alone), rounded once. */
int mi355_jagged_row_sum(const void* jagged, int64_t jagged_stride, const int64_t* offsets, int64_t batch, int64_t L, int64_t D,
                         void* out, int64_t out_stride, int dtype, hipStream_t stream);

/* ---- the FBGEMM sparse / jagged ops that examples/hstu calls as torch.ops.fbgemm.* (csrc/fbgemm_jagged.hip) ----
 * Reference paths below are relative to the reference's examples/.  Pure data movement: bit-exact, no read-modify-write
 * atomics, no host read, no allocation, capturable, 64-bit addressing.  `*_itype` is the type of an offsets / lengths / indices
 * vector: 0 = int32, 1 = int64 (read as they are, never converted).  Values are moved as bytes: `elem_bytes` is the element
 * size, not a dtype code. */

/* asynchronous_complete_cumsum / _inclusive_cumsum / _exclusive_cumsum (hstu/modules/jagged_data.py:125,133,142,
 * hstu/modules/hstu_processor.py:169,185, hstu/ops/jagged_tensor_op.py:60, commons/ops/length_to_offsets.py:20,25,30).
 * in: [rows, n] of int32 / int64 (`itype`).  mode 0 (complete): out is [rows, n + 1], out[r, 0] = 0 and out[r, i + 1] =
 * in[r, 0] + .. + in[r, i]; mode 1 (inclusive) and 2 (exclusive): out is [n], rows must be 1.  Sums wrap in the dtype as
 * torch.cumsum's do.  One pass over the data for any n: one block per row up to 8192 elements, above that a decoupled
 * look-back over 4096-element tiles, whose status words live in `workspace` (16-byte aligned,
 * mi355_cumsum_workspace_bytes(rows, n) bytes, 0 for the one-block case; contents irrelevant: the call clears them with a
 * small launch of its own in front of the scan).  A look-back launch holds one tile per block and no more tiles than the
 * device keeps resident (2 blocks per CU of the current device's CU count, about 2 M elements on 256 CUs); a longer input
 * takes further launches on the stream, each continuing from the output of the one before.  A block waits only for
 * lower-numbered blocks of its own launch, and every wait is bounded (seconds): if one ever runs out, the tiles concerned stay
 * UNWRITTEN, the call has long returned MI355_OK, and the only trace is the first 8 bytes of `workspace`, non-zero once the
 * stream has finished (zero after every healthy call).
 * rows == 0 or n == 0 launches nothing (the caller provides the [rows, 1] zeros of the complete sum). */
int64_t mi355_cumsum_workspace_bytes(int64_t rows, int64_t n);
int mi355_cumsum(const void* in, void* out, int64_t rows, int64_t n, int itype, int mode, void* workspace,
                 int64_t workspace_bytes, hipStream_t stream);

/* jagged_to_padded_dense / jagged_2d_to_dense (hstu/ops/jagged_tensor_op.py:66,105,111, hstu/ops/pt_ops/
 * pt_hstu_attention.py:117-137,247,257), and the backward of dense_to_jagged.  values: [T, D] with row stride D; offsets:
 * [B + 1]; out: [B, max_len, D] contiguous.  out[b, l, :] = values[offsets[b] + l, :] for l < min(len_b, max_len), else the
 * padding element, whose raw bits are `padding_bits` (the low elem_bytes bytes; so int64 -1 is as good as bf16 0.5); a sample
 * longer than max_len is truncated.  Every element of out is written exactly once, the padding included (no memset).
 * elem_bytes 2, 4 or 8; any D >= 1: 16-byte accesses where D elem_bytes and both base pointers allow, narrower otherwise.
 * A row index outside [0, T) (inconsistent offsets) reads nothing and gives padding. */
int mi355_jagged_to_padded(const void* values, int64_t T, const void* offsets, int offsets_itype, int64_t B, int64_t max_len,
                           int64_t D, int elem_bytes, uint64_t padding_bits, void* out, hipStream_t stream);

/* dense_to_jagged (hstu/ops/jagged_tensor_op.py:74,78 -- on the slices dense[:, :-n] and dense[:, n:] --,
 * hstu/ops/pt_ops/pt_hstu_attention.py:192), and the backward of the two to-dense ops.  dense: [B, N, D], element (b, l, d) at
 * dense + b stride_b + l stride_n + d (strides in ELEMENTS, inner dimension contiguous); out: [total, D] contiguous.
 * out[offsets[b] + l, :] = dense[b, l, :] for l < N, zeros for N <= l < len_b (FBGEMM allocates zeros).  Rows of out at or
 * past offsets[B] belong to no sample: they are written as zeros too (FBGEMM's zero allocation again, and what the backward of
 * jagged_to_padded_dense needs for value rows outside every sample), so every element of out is written exactly once. */
int mi355_padded_to_jagged(const void* dense, int64_t stride_b, int64_t stride_n, int64_t B, int64_t N, const void* offsets,
                           int offsets_itype, int64_t D, int elem_bytes, void* out, int64_t total, hipStream_t stream);

/* keyed_jagged_index_select_dim1 (commons/sequence_batch/batch.py:144, commons/distributed/batch_all2all.py:165,254,
 * commons/ops/collective_ops.py:602: the batch shuffler).  A KeyedJaggedTensor of F features x B samples: lengths [F B],
 * offsets [F B + 1], values [num_values]; indices [S] selects samples: output bag (f, j) is input bag (f, indices[j]).
 * mi355_kjt_select_lengths writes out_lengths [F S] (the type of lengths); its complete cumsum (mi355_cumsum, mode 0) is
 * out_offsets [F S + 1]; mi355_kjt_select_values then moves the bag contents into out_values [total] -- values of 1, 2, 4 or 8
 * bytes per element, and, when weights is non-null, weights (2, 4 or 8 bytes) into out_weights in the same launch.  One lane
 * per output element, so a bag of thousands of ids is spread like any other elements.
 * An index outside [0, B) yields an EMPTY bag (length 0, nothing moved): it is not a fault, and not undefined as it is in
 * FBGEMM.  Elements of out_values at or past out_offsets[F S], and elements whose source would lie outside its bag or outside
 * [0, num_values), are written as zeros; nothing outside the buffers is read or written whatever the vectors hold. */
int mi355_kjt_select_lengths(const void* lengths, int lengths_itype, const void* indices, int indices_itype, int64_t F,
                             int64_t B, int64_t S, void* out_lengths, hipStream_t stream);
int mi355_kjt_select_values(const void* values, int64_t num_values, int elem_bytes, const void* weights, int weight_bytes,
                            const void* offsets, int offsets_itype, const void* indices, int indices_itype, int64_t F,
                            int64_t B, int64_t S, const void* out_offsets, int out_offsets_itype, void* out_values,
                            void* out_weights, int64_t total, hipStream_t stream);

/* ---- beam-search decode attention of the semantic-ID generative-retrieval family (csrc/beam_decode.hip) ----
 * beam_decode_attn / BeamDecodeAttn (corelib/gr_decode_atten/interface.py:635-942; semantics: tests/reference.py there,
 * beam_attention_ref).  For batch b, beam w, query head h (kv head h / G, G = Hq / Hkv) the key set is the Sk_b context rows
 * of sample b followed by the beam rows k_beam[b, topk[b, 0, (h / G) G, n, w], h / G] for n < decode_nums; scores are
 * softmax_scale q.k; out = softmax(scores) V in `dtype` (1 = bf16, 2 = fp16, the type of every q / k / v), lse =
 * logsumexp(scores) in fp32.  A row with no key gives out = 0, lse = -inf.  A beam index outside [0, decode_nums W) is never
 * dereferenced: that key is absent.  A repeated index counts twice.
 *   q: element (b, w, h, d) at q + b q_stride_b + w q_stride_w + h q_stride_h + d; out [B, W, Hq, D] and lse [B, W, Hq] contiguous.
 *   context, dense (cu_seqlens_k null): [B, Sk, Hkv, D] at the given batch / row / head strides; Sk_b = Sk, or
 *     min(seqused_k[b], Sk) when seqused_k is non-null.  Jagged (cu_seqlens_k [B + 1] non-null): [total_k, Hkv, D], rows
 *     cu_seqlens_k[b] .. cu_seqlens_k[b + 1] (clamped to [0, total_k]); the batch strides and Sk are ignored.  seqused_k and
 *     cu_seqlens_k are mutually exclusive.
 *   beam: k_beam / v_beam [B, decode_nums W, Hkv, D] at the given strides; topk_indices (topk_itype 0 = int32, 1 = int64):
 *     element (b, 0, h, n, w) at b tk_stride_b + h tk_stride_h + n tk_stride_n + w tk_stride_w.
 * All strides are in elements; every q / k / v base pointer is 16-byte aligned and every q / k / v stride a multiple of 8.
 * D is 64 or 128.  num_splits >= 1 splits each sample's own key tiles (64 keys) into that many ranges, with any context
 * form; the fp32 partials live in `workspace` (16-byte aligned, mi355_beam_decode_workspace_bytes(B, W, Hq, D, num_splits)
 * bytes, contents irrelevant).  Two launches, no atomics: bitwise reproducible for a given num_splits.  No host read,
 * no allocation, capturable. */
int64_t mi355_beam_decode_workspace_bytes(int64_t B, int64_t W, int64_t Hq, int64_t D, int64_t num_splits);
int mi355_beam_decode_attn(const void* q, int64_t q_stride_b, int64_t q_stride_w, int64_t q_stride_h, const void* k_context,
                           const void* v_context, int64_t kc_stride_b, int64_t kc_stride_s, int64_t kc_stride_h,
                           int64_t vc_stride_b, int64_t vc_stride_s, int64_t vc_stride_h, int64_t Sk, int64_t total_k,
                           const int32_t* seqused_k, const int32_t* cu_seqlens_k, const void* k_beam, const void* v_beam,
                           int64_t kb_stride_b, int64_t kb_stride_s, int64_t kb_stride_h, int64_t vb_stride_b,
                           int64_t vb_stride_s, int64_t vb_stride_h, const void* topk_indices, int topk_itype,
                           int64_t tk_stride_b, int64_t tk_stride_h, int64_t tk_stride_n, int64_t tk_stride_w, int64_t B,
                           int64_t W, int64_t Hq, int64_t Hkv, int64_t D, int64_t decode_nums, float softmax_scale,
                           int64_t num_splits, void* out, float* lse, int dtype, void* workspace, int64_t workspace_bytes,
                           hipStream_t stream);

/* ---- softmax prefill attention of the semantic-ID generative-retrieval family, forward (csrc/prefill_attn.hip) ----
 * Replaces the flash-attention calls of examples/sid_gr/model/jagged_flash_attn_block.py and of sid-gr-inference's
 * gr_kernels/prefill/flash_attn_backend.py: flash_attn.flash_attn_interface.flash_attn_varlen_func(q, k, v, cu_seqlens_q,
 * cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale, causal), flash_attn.flash_attn_func(q, k, v, softmax_scale, causal)
 * and flash_attn.cute.interface.flash_attn_func(..., arbitrary=True, aux_tensors=[arbitrary_func]).
 * For sequence b and query head h (kv head h / G, G = Hq / Hkv) with Lq queries and Lk keys, query i sees key j iff
 *   mask 0 (none):    always;
 *   mask 1 (causal):  j <= i + Lk - Lq (bottom-right aligned, flash-attn >= 2.1; a row with i + Lk - Lq < 0 sees nothing);
 *   mask 2 (func):    j < F[0][i], or F[2p-1][i] <= j < F[2p][i] for some p >= 1 (interval ends clamped to [0, Lk], an interval
 *                     with start >= end is empty), F = func[b, h or 0]: element (b, h, f, i) at func + b func_stride_b +
 *                     h func_stride_h + f func_stride_f + i func_stride_s, int32, n_func odd, func_heads 1 or Hq; columns at or
 *                     past Sq are never read.  Dense form only; func must be null for masks 0 and 1.
 * scores = softmax_scale q.k; out = softmax(scores) V in `dtype` (1 = bf16, 2 = fp16, the type of q, k and v); lse =
 * logsumexp(scores), natural log, fp32.  A row with no visible key gives out = 0 and lse = -inf exactly.
 *   dense (cu_seqlens_q = cu_seqlens_k = null): q [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] at the given batch / row / head strides;
 *     out [B, Sq, Hq, D] and lse [B, Hq, Sq] contiguous.  total_q / total_k are ignored.
 *   jagged (both non-null, int32 [B + 1]): q [total_q, Hq, D], k / v [total_k, Hkv, D] at the given row / head strides (the
 *     batch strides and Sk are ignored); sequence b is rows cu[b] .. cu[b + 1], the bounds clamped into [0, total] and made
 *     monotone, so that no row outside the tensors is read.  Sq is max_seqlen_q: query rows of a sequence at or past it are
 *     not computed.  out [total_q, Hq, D] and lse [Hq, total_q] contiguous.
 * All strides are in elements; every q / k / v / out base pointer is 16-byte aligned and every q / k / v stride a multiple of
 * 8 (so views of one packed [B, S, 3, H, D] buffer are taken as they are).  D is 64 or 128.  skip_tiles: 1 (the default of
 * the Python surface) visits only the key tiles (64 keys) that the rows of a workgroup (128 query rows) can see; 0 visits and
 * tests all of them, with bitwise the same result.  One launch, no workspace, no atomics, no host read: capturable and bitwise reproducible. */
int mi355_prefill_attn(const void* q, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, const void* k,
                       int64_t k_stride_b, int64_t k_stride_s, int64_t k_stride_h, const void* v, int64_t v_stride_b,
                       int64_t v_stride_s, int64_t v_stride_h, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                       int64_t B, int64_t Sq, int64_t Sk, int64_t total_q, int64_t total_k, int64_t Hq, int64_t Hkv, int64_t D,
                       int mask, const int32_t* func, int64_t n_func, int64_t func_heads, int64_t func_stride_b,
                       int64_t func_stride_h, int64_t func_stride_f, int64_t func_stride_s, float softmax_scale,
                       int skip_tiles, void* out, float* lse, int dtype, hipStream_t stream);

/* ---- softmax attention backward: dq, dk, dv of mi355_prefill_attn (csrc/softmax_attn_bwd.hip) ----
 * The training side of the same three flash-attention calls (examples/sid_gr/model/jagged_flash_attn_block.py runs them under
 * autograd).  The arguments up to skip_tiles are those of mi355_prefill_attn with the same meaning (forms, strides, masks,
 * clamped cu_seqlens); in the jagged form Sk carries max_seqlen_k, which bounds the dK / dV launch the way Sq = max_seqlen_q
 * bounds the forward's: both must be at least the longest sequence.
 *   out   the forward's output, contiguous ([B, Sq, Hq, D] / [total_q, Hq, D]);
 *   dout  its gradient, same shape, at the given batch / row / head strides (batch ignored in the jagged form), rows 16-byte aligned;
 *   lse   the forward's, fp32 natural log ([B, Hq, Sq] / [Hq, total_q]);
 *   delta workspace, fp32, the shape of lse: written (delta_i = sum_d dout_id out_id) by the first launch, read by the second;
 *   dq [B, Sq, Hq, D] / [total_q, Hq, D], dk and dv [B, Sk, Hkv, D] / [total_k, Hkv, D]: contiguous, in `dtype`.
 * P is recomputed from lse, dS = P (dP - delta); P and dS are rounded once to `dtype` for the products, sums are fp32, each
 * gradient is rounded once.  dk / dv of a kv head sum over its Hq / Hkv query heads in head order inside one workgroup.
 * Every element of dq / dk / dv that belongs to a sequence is written (the caller zeroes nothing): a row with lse = -inf gets
 * dq = 0 and a key no query sees dk = dv = 0 exactly.  n_func is at most 129.  skip_tiles = 0 gives bitwise the same result.
 * Two launches, no atomics, no allocation, no host read: capturable and bitwise reproducible. */
int mi355_softmax_attn_bwd(const void* q, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, const void* k,
                           int64_t k_stride_b, int64_t k_stride_s, int64_t k_stride_h, const void* v, int64_t v_stride_b,
                           int64_t v_stride_s, int64_t v_stride_h, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                           int64_t B, int64_t Sq, int64_t Sk, int64_t total_q, int64_t total_k, int64_t Hq, int64_t Hkv, int64_t D,
                           int mask, const int32_t* func, int64_t n_func, int64_t func_heads, int64_t func_stride_b,
                           int64_t func_stride_h, int64_t func_stride_f, int64_t func_stride_s, float softmax_scale,
                           int skip_tiles, const void* out, const void* dout, int64_t dout_stride_b, int64_t dout_stride_s,
                           int64_t dout_stride_h, const float* lse, float* delta, void* dq, void* dk, void* dv, int dtype,
                           hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RECSYS_AMD_H_ */
