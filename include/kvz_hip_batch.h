/*
 * kvz_hip_batch.h -- batched, device-resident entry points of libkvz_hip.so (group 3 of kvz_hip.h).
 *
 * The per-call strategy functions (kvz_hip.h) are bit-exact drop-ins but pay a PCIe round trip per call; kvazaar
 * makes ~3 500 such calls per CTU.  The throughput path keeps whole batches of frames in HBM and runs kvazaar's
 * per-CTU flow (search.c:1209 kvz_search_lcu and everything below it that SURVEY.md section 8a lists for the
 * all-intra `ultrafast` configuration: angular / planar / DC prediction, SATD mode costs, DCT 4..32, quantisation,
 * dequantisation, IDCT, reconstruction, SSD and fast coefficient cost) as ONE workgroup per CTU out of LDS.
 *
 * Frame independence: with `-p 1` every frame is an IDR picture (encoderstate.c:1599-1620), so a batch of N frames
 * is N independent problems; inside a frame CTU (x, y) needs its left, above and above-right neighbours, i.e. the
 * WPP order of encoderstate.c:793-903.  One persistent kernel launch per call draws the CTUs of EVERY frame of the batch from a
 * ticket list in that order (anti-diagonals x + 2y = const; raster order per picture when the model says no WPP) and workgroups
 * hand results to each other through per-CTU border records.
 *
 * Decisions use kvazaar's own cost formulas, in double precision with the reference's operation order, on CABAC contexts
 * that evolve as kvazaar's do (kvz_hip_intra_cost_model): the reconstruction, CU quadtree, modes and coefficients
 * are those of `kvazaar --preset ultrafast -p 1`, picture for picture (tests/test_encoder_parity.py checks the pass against
 * digests of the reference CLI's --debug output).  The checker for every intermediate is oracle/kvz_oracle_ctu.c.
 */
#ifndef KVZ_HIP_BATCH_H_
#define KVZ_HIP_BATCH_H_

#include "kvz_hip_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kvz_hip_batch kvz_hip_batch; /* device buffers for n_frames pictures of width x height (yuv420p, 8 bit) */

/* width and height must be multiples of 8 (kvazaar pads its input the same way).  NULL on failure. */
kvz_hip_batch *kvz_hip_batch_create(int width, int height, int n_frames);
/* ... on a given device (0 .. kvz_hip_device_count() - 1; -1 = the calling thread's current one, which is what kvz_hip_batch_create does).  The reference runs the
 * tiles of a picture as jobs of ONE process (encoderstate.c:944-1013 builds one sub-encoder per tile, threadqueue.c:275-355 runs them on its workers): a host that
 * wants tile i on GPU i % count creates tile i's batch with this and calls it from any thread -- every entry point taking a kvz_hip_batch binds the calling thread
 * to the batch's device first, and its buffers, stream and kernels stay there.  NULL when the device does not exist. */
kvz_hip_batch *kvz_hip_batch_create_on(int device, int width, int height, int n_frames);
void           kvz_hip_batch_destroy(kvz_hip_batch *b);

/* Host <-> HBM.  Planes are tightly packed (stride = width; chroma width/2 x height/2). */
void kvz_hip_batch_upload(kvz_hip_batch *b, int frame, const uint8_t *y, const uint8_t *u, const uint8_t *v);
/* All n_frames pictures at once, asynchronously: `src` holds them back to back, each Y | U | V tightly packed (kvz_image_alloc's planar buffer, image.c:62-95),
 * preferably in kvz_hip_host_alloc'ed memory.  The copy runs on a queue of its own and starts when the batch's LAST pass has ended -- the pass is the only reader
 * of the source pictures (SAO's statistics aside: not while kvz_hip_batch_loop_filters with sao is in flight) -- so it overlaps the batch's own deblocking and
 * entropy coding and another batch's pass; the batch's NEXT kvz_hip_intra_frames waits for it.  `src` must stay untouched until that pass has been synced.
 * What a host feeding the device from its reader thread (encoder.c / input frame queue) does per batch instead of n_frames synchronous uploads.
 * All batches of a device share ONE upload queue.  The HIP runtime runs a process's streams on GPU_MAX_HW_QUEUES hardware queues (default 4) and streams sharing one
 * wait for each other: a double-buffered chain (two batches, the entropy coder's side stream, the upload queue, the calling thread's own stream) needs more, so the
 * library sets GPU_MAX_HW_QUEUES=8 when it is loaded unless the variable is already set -- effective when that happens before the process's first HIP call. */
void kvz_hip_batch_upload_all_async(kvz_hip_batch *b, const uint8_t *src);
/* Any output pointer may be NULL.  coeff: KVZ_HIP_CTU_COEFFS int16 per CTU (raster CTU order, lcu_t z-order inside);
 * cu_depth / cu_mode: one byte per 8x8 block (raster, stride width/8); ctu_cost: one double per CTU.
 * Returns 0, or -1 when the run that produced the data was invalid (see kvz_hip_batch_sync). */
int  kvz_hip_batch_download(kvz_hip_batch *b, int frame, uint8_t *rec_y, uint8_t *rec_u, uint8_t *rec_v, int16_t *coeff,
                            uint8_t *cu_depth, uint8_t *cu_mode, double *ctu_cost);

/* After a pass with model.search_nxn: cu_part, one byte per 8x8 block (raster, stride width/8): 1 = the CU is coded as four 4x4 prediction units (part_size NxN);
 * cu_mode4, the luma mode of every 4x4 unit (raster, stride width/4; four equal entries for a 2Nx2N CU -- cu_mode of kvz_hip_batch_download holds the first PU's).
 * Either may be NULL.  Returns 0, or -1 when the run was invalid or no such pass has run on the batch. */
int  kvz_hip_batch_download_partitions(kvz_hip_batch *b, int frame, uint8_t *cu_part, uint8_t *cu_mode4);

/* Pinned host memory (hipHostMalloc) for the asynchronous transfers below; plain malloc'ed buffers work too but serialise. */
void *kvz_hip_host_alloc(size_t bytes);
void  kvz_hip_host_free(void *p);
/* Queues the download of what the entropy coder needs of EVERY frame of the batch (encode_coding_tree.c:745 reads the coefficients,
 * cu_info and -- for the next stages -- the reconstruction) on the batch's stream, behind whatever it holds: with pinned
 * destinations the copies overlap the kernels of other batches' streams (two batches alternating = double buffering).
 * Layouts as kvz_hip_batch_download, frames back to back; NULL skips a buffer.  kvz_hip_batch_sync() waits and validates. */
void kvz_hip_batch_download_all_async(kvz_hip_batch *b, uint8_t *rec, int16_t *coeff, uint8_t *cu_depth, uint8_t *cu_mode);

/* Work queued on `b` from now on starts only after everything queued on `other` so far has finished (both on the same device).  The
 * CTU pass is ONE persistent launch that takes every workgroup slot of the device until its tickets run out: a second batch's pass launched
 * right behind it moves into the slots as they free up, and the first batch's small follow-up kernels (deblocking, SAO, checksums) then wait
 * for the whole second pass -- and with them its download.  Double-buffered pipelines therefore order the next batch's pass after the
 * previous batch's follow-up kernels, and queue the download behind that point (bench.py chain_d2h): the copy engines then run during
 * the next pass. */
void kvz_hip_batch_order_after(kvz_hip_batch *b, kvz_hip_batch *other);
/* The share of the device this batch's persistent pass takes: `num` of every `den` workgroup slots per CU (1 <= num <= den; (1, 1) = all of them, the default).
 * Batches of different geometry that are meant to run side by side -- the two tile sizes of kvazaar's uniform tile grid (encoderstate.c:944-979: 960x1088 and
 * 960x1072 at 3840x2160 --tiles 4x2) -- each take their share; with the default the first launch fills the device and the second one only moves in when the
 * first one's workgroups retire, i.e. the two passes run one after the other, each on fewer serial CTU chains than the device has slots.  Takes effect with
 * the next kvz_hip_intra_frames. */
void kvz_hip_batch_set_device_share(kvz_hip_batch *b, int num, int den);

/* The hot path: search + reconstruct every CTU of every frame in the batch.  Asynchronous on the batch's stream;
 * kvz_hip_batch_sync() waits.  Returns the number of kernel launches issued (1; one per CTU anti-diagonal with the older
 * schedule behind KVZ_HIP_SCHED=wave), or -1 -- with a message on stderr and nothing launched -- for a model the batch cannot run (rdoq without coeff_cabac;
 * search_32x32 / rdoq / search_nxn / no_wpp under KVZ_HIP_SCHED=wave). */
int  kvz_hip_intra_frames(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model);
/* Waits for the batch's stream.  Returns 0, or -1 when a CTU hand-off wait inside a pass timed out (workgroups wait for their
 * neighbours' results with a wall-clock bound -- 30 s per wait, KVZ_HIP_WAIT_MS overrides -- so that a lost hand-off cannot hang
 * the GPU): the batch's results are then invalid and every later sync / download / checksum call of the batch reports -1 too.
 * HIP runtime failures (no device, out of memory, launch failure) stay fatal, as in the per-call path. */
int  kvz_hip_batch_sync(kvz_hip_batch *b);
/* After a pass reported -1: once a hand-off wait has timed out the rest of that pass only drains its tickets (no CTU is searched on stale neighbour data, nothing
 * waits again) and the batch stays invalid -- sticky, so that no later call can mistake its contents for results -- until this call clears the condition.  The
 * pictures uploaded to the batch are untouched: the caller may simply run the pass again.  Returns 0. */
int  kvz_hip_batch_reset(kvz_hip_batch *b);
/* developer diagnostics: every CTU's hand-off flag (= the number of the last pass that completed it) into out [n_frames x CTUs per frame]; returns the number of the batch's last pass */
unsigned kvz_hip_batch_debug_flags(kvz_hip_batch *b, unsigned *out);
/* Device time of the launches of the last kvz_hip_intra_frames call, from HIP events recorded on the batch's own
 * stream around the launch sequence (milliseconds); call after kvz_hip_batch_sync(). */
float kvz_hip_batch_last_kernel_ms(kvz_hip_batch *b);
int   kvz_hip_batch_ctus_per_frame(const kvz_hip_batch *b);
/* Developer aid: per-stage shader-cycle counters of a -DKVZ_CTU_PROFILE build of the library (zeros otherwise). */
int   kvz_hip_batch_profile(kvz_hip_batch *b, unsigned long long *out, int n);

/* Deblocks the batch's reconstruction in place on the batch's stream (kvz_filter_deblock_lcu, filter.c:783, over every LCU of
 * every frame; see kvz_hip_dev_deblock_frames in kvz_hip_dev.h) using the CU depths the last kvz_hip_intra_frames() left.
 * kvazaar runs it right after an LCU's reconstruction (encoderstate.c:669-671); downloads after this call return the
 * deblocked picture.  The next kvz_hip_intra_frames() overwrites the reconstruction. */
void kvz_hip_batch_deblock(kvz_hip_batch *b, int qp, int beta_offset_div2, int tc_offset_div2);

/* Both in-loop filters the way the encoder runs them per LCU (encoderstate.c:669-682): deblocking (when `deblock`) and -- when `sao` --
 * the SAO parameter decision kvz_sao_search_lcu (sao.c:671, `--sao full`: edge and band) on the partly deblocked picture each LCU sees at
 * that moment, with the merge-left / merge-up choice and the bit costs on the two SAO contexts as the LCU's real syntax moves them
 * (encoderstate.c:467-552), followed by kvz_sao_reconstruct (sao.c:302-361) of every LCU.  On the batch's stream; afterwards the batch's
 * reconstruction is the final picture (what `kvazaar --debug` writes), the decided parameters are read with kvz_hip_batch_sao_params().
 * model: the cost model of the CTU pass (lambda, entropy table, no_wpp, the SAO contexts' initial states in ctx_init).  With sao == 0 this
 * is kvz_hip_batch_deblock.  Three statistic sets per LCU (4 edge classes x 5 categories, 32 bands: {sum, count}) are gathered by one
 * workgroup per (LCU, plane); the decision chain -- serial per picture like the coder it follows -- runs one lane per picture. */
void kvz_hip_batch_loop_filters(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int deblock, int beta_offset_div2, int tc_offset_div2, int sao);
/* The SAO parameters of one frame as the last kvz_hip_batch_loop_filters(..., sao = 1) decided them: one record per LCU in raster order
 * (chroma: U in offsets[0..4] / band_position[0], V in offsets[5..9] / band_position[1], like sao_info_t); merge: 0 none, 1 left, 2 up.
 * LCUs whose type is 0 (none) carry zeros in the other fields.  Any pointer may be NULL.  0 / -1 like kvz_hip_batch_sync. */
int  kvz_hip_batch_sao_params(kvz_hip_batch *b, int frame, kvz_hip_sao_params *luma, kvz_hip_sao_params *chroma, uint8_t *merge);

/* Picture-hash checksums (nal.c:73-86 kvz_image_checksum) of every frame's current reconstruction: host_out[3 * f + plane].
 * Queued behind whatever the batch's stream holds (CTU pass, deblocking) and waited for. */
int  kvz_hip_batch_checksums(kvz_hip_batch *b, uint32_t *host_out);  /* 0 / -1 like kvz_hip_batch_sync */

/* ... and the MD5 flavour of the picture hash (nal.c:88-101 kvz_image_md5, `--hash md5`): host_out[(3 f + plane) * 16 ..] = 16 digest bytes. */
int  kvz_hip_batch_md5(kvz_hip_batch *b, uint8_t *host_out);

/* Distortion of every frame: host_out[3 * f + plane] = the exact sum of squared differences between the frame's source picture and its reconstruction as the
 * batch holds it NOW -- after kvz_hip_batch_deblock / _loop_filters if they ran: kvazaar's PSNR (encmain.c:117-145 compute_psnr, the `PSNR Y U V` of its log
 * line, cli.c:721-753) is of the final picture.  kvz_hip_psnr (kvz_hip.h) turns a sum into that figure.  Both pictures are read where they are (3 x w h bytes
 * per frame, kvz_hip_dev_picture_sse) and 24 bytes per frame come back: the rate of a picture is the size of its slice data (kvz_hip_batch_entropy_code), this
 * is the other half.  Queued behind whatever the batch's stream holds and waited for; 0 / -1 like kvz_hip_batch_checksums (-1 also for a NULL argument). */
int  kvz_hip_batch_sse(kvz_hip_batch *b, uint64_t *host_out);
/* ... queued on the batch's stream without waiting: host_out (kvz_hip_host_alloc'ed memory, or the copy is not asynchronous) is valid after kvz_hip_batch_sync.
 * Returns 0, or -1 for a NULL argument (nothing queued).
 * Ordering against kvz_hip_batch_upload_all_async, which replaces the source pictures on a queue of its own: A SUM QUEUED BEFORE AN UPLOAD SEES THE OLD
 * PICTURES, ONE QUEUED AFTER IT THE NEW ONES.  The upload starts behind the last sum queued so far (and behind the last pass, as always); a sum queued after an
 * upload waits for it, as the next pass does.  (kvz_hip_batch_upload copies on the batch's own stream and is ordered by it.)  With no sum queued, uploads wait for
 * exactly what they waited for before. */
int  kvz_hip_batch_sse_async(kvz_hip_batch *b, uint64_t *host_out);

/* Cost model of an I slice at `qp` (kvz_hip_intra_cost_model, adaptive contexts): HEVC context init values
 * (context.c:96-134), kvz_ctx_init (context.c:202-213), the HM entropy table (rdo.c:69-80), lambda of
 * rate_control.c:678-691.  coeff_weights = kvz_fast_coeff_get_weights(state) of the encoder (fast_coeff_cost.c:84-88). */
void kvz_hip_intra_cost_model_init(int qp, uint64_t coeff_weights, kvz_hip_intra_cost_model *model);
/* kvz_fast_coeff_get_weights for kvazaar's built-in table (fast_coeff_cost.h:48-101 packed by fast_coeff_cost.c:39-52); 0 for
 * QP >= MAX_FAST_COEFF_COST_QP (50), where kvazaar never uses the fast estimate (rdo.c:311-340). */
/* The entropy coder in its REAL mode -- what kvazaar's encoder_state_worker_encode_lcu_bitstream writes (encoderstate.c:676-745: SAO syntax, kvz_encode_coding_tree
 * encode_coding_tree.c:745, kvz_encode_coeff_nxn strategies/generic/encode_coding_tree-generic.c:40, the arithmetic coder cabac.c:85-270, the per-substream flush and
 * byte alignment) for every picture of the batch, on the device, from the results of the last kvz_hip_intra_frames (CU depths / modes / partitions, levels) and -- with
 * sao != 0 -- of the last kvz_hip_batch_loop_filters(..., sao = 1): I slices of the configurations the pass covers.  model: the pass's (ctx_init = the slice's initial
 * context states, no_wpp, search_nxn).  out (HOST, `capacity` bytes) receives the slice data: picture after picture, and inside a picture one substream per CTU row
 * (WPP; the rows' contexts start from the row above after its second CTU, encoderstate.c:763-771) or one for the whole picture (no_wpp); substream_bytes (HOST) their sizes,
 * n_frames x (CTU rows | 1) entries -- the entry points of the slice header (encoder_state-bitstream.c:935-954).  The bytes are those of kvazaar's per-row bitstream_t
 * objects, emulation prevention bytes included (bitstream.c:212-223): what follows the slice header in the NAL unit, verbatim.  Only these bytes cross PCIe instead of
 * the levels (12 KB per CTU).  Returns the total size, -1 on failure. */
long kvz_hip_batch_entropy_code(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int sao, uint8_t *out, size_t capacity, uint32_t *substream_bytes);
/* ... when the batch's pictures are TILES of larger pictures (each tile a picture of its own for the pass, model.no_wpp as kvazaar codes tiles): not_last[f] != 0 (HOST,
 * n_frames entries) marks a tile that is not the last of its slice -- its substream ends in end_of_subset_one_bit instead of end_of_slice_segment_flag
 * (encoderstate.c:699-724).  not_last == NULL: every picture is a slice of its own (the function above). */
long kvz_hip_batch_entropy_code_tiles(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                      uint32_t *substream_bytes);
/* ... and a pipeline's form of it: once the coder's first stage is through and its third is queued -- a few hundred wavefronts that each follow one substream's chain,
 * then the download: the device is nearly idle from there on --, the CTU pass of `next` is started with `next_model` (kvz_hip_intra_frames(next, next_model); another
 * batch on the same device), so that it runs beside the rest of this call.  Started any earlier, the pass -- one persistent launch that takes every workgroup slot it
 * finds -- would keep the coder's first stage, which wants the whole device, waiting until it is done.  next == NULL: kvz_hip_batch_entropy_code_tiles.
 * Returns: the total size; -1 the coder failed (as kvz_hip_batch_entropy_code_tiles); -2 the coder succeeded but kvz_hip_intra_frames(next, next_model) returned an
 * error; -3 next_model is NULL or of an unknown struct_size -- checked first, nothing has been queued on either batch.  In every other case, -1 and -2 included,
 * `next`'s pass HAS been queued exactly once when the call returns (at the coder's quiet moment, or at the end of the call when the coder never reached it): the
 * caller synchronises `next` (kvz_hip_batch_sync) whatever this call returned. */
long kvz_hip_batch_entropy_code_then(kvz_hip_batch *b, const kvz_hip_intra_cost_model *model, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                     uint32_t *substream_bytes, kvz_hip_batch *next, const kvz_hip_intra_cost_model *next_model);
/* With `on` != 0 the three calls above return on this batch as soon as the slice data's download has been QUEUED on the batch's stream (the substream sizes are final and
 * the return value is the total; the bytes in `out` -- pinned memory, or the copy is not asynchronous -- are valid after kvz_hip_batch_sync(b) or the batch's next call
 * that synchronises its stream).  In a pipeline of two batches in turn the next batch's deblocking and coder then start while this batch's 0.4 MB per picture are still
 * on their way down (13 ms per 1 536 1080p pictures that sat between two passes).  The batch compacts into a device buffer of its own in this mode. */
void kvz_hip_batch_entropy_defer_download(kvz_hip_batch *b, int on);
uint64_t kvz_hip_default_coeff_weights(int qp);

/* ---- Pictures under different cost models in one launch (kvz_hip_picture_models, kvz_hip_types.h) ----
 * The entry points above take ONE model -- one QP, one lambda, one set of initial context states -- for the whole batch; pictures of streams at different QPs would have
 * to go in one small launch per QP, the latency-bound regime the batch exists to avoid.  These mirror them one for one with a model per picture.  Each picture's
 * outputs are those of the single-model call on a batch of that picture's QP; a table of one model is the single-model call.  Every one of them returns -1 (the loop
 * filters: mark the batch failed, kvz_hip_batch_sync -> -1) with a message on stderr and NOTHING queued for: a struct_size this library does not know, of the table or
 * of any model; n_models < 1; a model index out of range; models that disagree in adaptive / no_wpp / search_32x32 / rdoq / search_nxn / entropy_fbits; rdoq with
 * a model without coeff_cabac; the KVZ_HIP_SCHED=wave schedule.  The table is kept in a device buffer of the batch and copied only when it differs from the last
 * call's: a steady chain of calls with one table pays one copy.
 * The pass runs the instantiation with the CABAC coefficient model when ANY model has coeff_cabac; pictures whose model has not are priced by the fast estimate
 * through that instantiation's run-time switch. */
int  kvz_hip_intra_frames_models(kvz_hip_batch *b, const kvz_hip_picture_models *models);
/* kvz_hip_batch_loop_filters (with sao == 0: kvz_hip_batch_deblock) with every picture's own QP in the deblocking thresholds and its own lambda and SAO contexts in the
 * SAO decision. */
int  kvz_hip_batch_loop_filters_models(kvz_hip_batch *b, const kvz_hip_picture_models *models, int deblock, int beta_offset_div2, int tc_offset_div2, int sao);
/* kvz_hip_batch_entropy_code_tiles (not_last == NULL: kvz_hip_batch_entropy_code): every substream starts from its picture's own initial context states.  Nothing else in
 * the slice data depends on the QP; parameter sets and slice headers (slice_qp_delta) stay with the host. */
long kvz_hip_batch_entropy_code_models(kvz_hip_batch *b, const kvz_hip_picture_models *models, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                       uint32_t *substream_bytes);
/* kvz_hip_batch_entropy_code_then with tables: `next`'s pass is kvz_hip_intra_frames_models(next, next_models).  Same contract: -3 (nothing queued on either batch) when
 * next != NULL and next_models is not a table `next` can run; in every other case, -1 and -2 included, `next`'s pass has been queued exactly once when the call
 * returns -- also when `models` is a table `b` cannot run (-1, nothing queued on `b`). */
long kvz_hip_batch_entropy_code_then_models(kvz_hip_batch *b, const kvz_hip_picture_models *models, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity,
                                            uint32_t *substream_bytes, kvz_hip_batch *next, const kvz_hip_picture_models *next_models);

/* ---- A cost model per CTU: cu_qp_delta (kvz_hip_ctu_models, kvz_hip_types.h) ----
 * kvz_hip_intra_frames_models with a model per CTU instead of a model per picture: every CTU is searched, quantised, priced and reconstructed under the qp, lambda,
 * lambda_sqrt, coeff_weights and coeff_cabac of the row model_of_ctu names; its picture's slice model supplies ctx_init and the switches.  A map that repeats each
 * picture's own model gives what kvz_hip_intra_frames_models gives, byte for byte.  Behind the pass, on the batch's stream, the call derives the QP every CU ends up
 * with (encoderstate.c:574-633 set_cu_qps with max_qp_delta_depth 0, one quantisation group per CTU).  A substream's predictor `last` starts at the slice QP at the
 * start of every CTU row (no_wpp: once per picture, running through the rows in raster order); for each CTU pred = last, the CUs in coding order before the first CU
 * with any coded block flag take QP pred, that CU and all after it the CTU's QP Q, and afterwards last = Q if the CTU has a coefficient anywhere, else pred.  Q - pred is
 * the cu_qp_delta the first transform unit with a coded block flag carries.
 * Returns 1, or -1 with a message on stderr, NOTHING queued and the batch usable as before for: a struct_size this library does not know, a NULL member, a map index
 * >= n_models; everything kvz_hip_intra_frames_models refuses; any model with rdoq, search_nxn or signhide; a batch that has scaling lists; KVZ_HIP_SCHED=wave; a picture
 * whose QPs (slice QP and every CTU QP) span more than 25 -- which CTU predicts which depends on results, so the pairwise bound is what keeps every delta codable.
 * Not built: tiles, batch groups, the inter path, preset `medium`; computing --vaq offsets or a rate controller's lambdas is the caller's business (it brings the map). */
int  kvz_hip_intra_frames_ctu_models(kvz_hip_batch *b, const kvz_hip_ctu_models *cm);
/* What the last kvz_hip_intra_frames_ctu_models derived for picture `frame` (after the stream has drained; any pointer may be NULL): cu_qp [(H/8)*(W/8)] the QP of
 * every 8x8 unit, raster like cu_depth; ctu_qp [CTUs, raster] per CTU pred | Q << 8 | coded << 16 | first << 24 -- coded: the CTU has a coefficient, so a delta
 * (0 included) is coded; first: the z-order index of the first 8x8 unit of the first CU with a coded block flag (64: none).  -1: no such pass has run on the batch, or
 * the batch's last pass was invalid. */
int  kvz_hip_batch_download_cu_qps(kvz_hip_batch *b, int frame, uint8_t *cu_qp, uint32_t *ctu_qp);
/* device time of the CU-QP step behind the last kvz_hip_intra_frames_ctu_models (milliseconds; kvz_hip_batch_last_kernel_ms is the pass alone); call after a sync */
float kvz_hip_batch_last_cu_qp_ms(kvz_hip_batch *b);
/* kvz_hip_batch_loop_filters_models after kvz_hip_intra_frames_ctu_models with the same `cm`: every edge part is filtered at (QpP + QpQ + 1) >> 1 of the two CU QPs
 * the pass left (filter.c:275-295); that value gives beta and tc, and the chroma tc through the chroma QP table.  The SAO decision of a CTU uses that CTU's lambda;
 * its two contexts start from the slice QP.  -1 with a message and nothing queued for what kvz_hip_intra_frames_ctu_models refuses, when the batch's last pass
 * was no such pass (the CU QPs come from it), and when `cm` is not that pass's map (another lambda, row or QP for any CTU: the lambdas and the CU QPs belong together).
 */
int  kvz_hip_batch_loop_filters_ctu_models(kvz_hip_batch *b, const kvz_hip_ctu_models *cm, int deblock, int beta_offset_div2, int tc_offset_div2, int sao);

/* kvz_hip_batch_entropy_code_models after kvz_hip_intra_frames_ctu_models with the same `cm` (not_last must be NULL: no tiles): Q - pred of a CTU is coded in the first
 * transform unit of the CTU that has a coded block flag (encode_coding_tree.c:282-305) -- cu_qp_delta_abs with a truncated-unary prefix, cMax 5, the first bin on
 * context 0 and the others on context 1, and an EG0 suffix of |d| - 5 in bypass bins; cu_qp_delta_sign_flag as one bypass bin when d != 0.  The two contexts start
 * from init value 154 at the slice QP; the library derives them, kvz_hip_intra_cost_model keeps its size.  Slice header, PPS (cu_qp_delta_enabled_flag,
 * diff_cu_qp_delta_depth 0) and NAL framing stay with the host.  -1 with a message and nothing queued for what kvz_hip_intra_frames_ctu_models refuses, for
 * not_last != NULL, when the batch's last pass was no such pass and when `cm` is not that pass's map. */
long kvz_hip_batch_entropy_code_ctu_models(kvz_hip_batch *b, const kvz_hip_ctu_models *cm, int sao, const uint8_t *not_last, uint8_t *out, size_t capacity, uint32_t *substream_bytes);

/* ---- Per-coefficient scaling lists (kvz_hip_scaling_lists, kvz_hip_types.h) ----
 * kvazaar's --scaling-list default: H.265 tables 7-5 and 7-6 (scalinglist.c:266-282), every DC term 16. */
void kvz_hip_scaling_lists_default(kvz_hip_scaling_lists *lists);
/* Gives the batch n_sets list sets and each picture one of them: set_of_picture[n_frames of the batch] (HOST) holds an index below n_sets, or 0xffff for a picture
 * that stays flat; NULL: every picture uses set 0.  n_sets == 0 clears the state: the batch is then what it was before the first such call.  The arrays are copied
 * (the forward factors (quant_scale << 4) / entry and the inverse ones inv_quant_scale * entry are derived here, once per set and qp % 6).  State of the batch like
 * kvz_hip_batch_set_device_share: it holds for every later kvz_hip_intra_frames and kvz_hip_intra_frames_models on the batch (also the passes
 * kvz_hip_batch_entropy_code_then[_models] start on it as `next`), with each picture's luma factors taken at its model's qp % 6 and its chroma factors at its chroma QP's.
 * Pictures with lists and pictures without share one launch; a flat picture of such a launch comes out byte for byte as in a launch on a batch without lists, and a
 * batch without lists launches the kernels it launched before.  Loop filters, SAO, hashes, distortion and the entropy coder do not depend on lists (the lists
 * themselves are SPS / PPS syntax and stay with the host).
 * The factor rows and one word per picture (its two rows at its QP) are kept in a device buffer of the batch and staged by the pass like the model table of
 * kvz_hip_intra_frames_models: compared with what the device holds on every launch and copied -- a small copy the call waits for -- only when the sets, a picture's set or a
 * picture's QP changed since the last launch; a steady chain of launches pays one copy.  (A pass started as `next` by kvz_hip_batch_entropy_code_then pays that wait inside
 * the overlap when its QPs change from launch to launch.)
 * Returns 0, or -1 -- with a message on stderr and the batch's previous state kept -- for: a struct_size this library does not know; an entry or a non-zero DC term
 * outside 13 .. 255; a set index that is neither below n_sets nor 0xffff; n_sets < 0 or > 65535, or sets == NULL with n_sets > 0; a batch under KVZ_HIP_SCHED=wave.
 * While a batch has lists, a pass whose model (any model of a table) has rdoq, search_nxn or signhide is refused: -1, a message that names scaling lists, nothing
 * queued.  (kvz_rdoq with lists needs the per-coefficient error scales of scalinglist.c:351-367, the hiding rule a factor per position: neither is built.) */
int  kvz_hip_batch_set_scaling_lists(kvz_hip_batch *b, const kvz_hip_scaling_lists *sets, int n_sets, const uint16_t *set_of_picture);

/* ---- Batches of different picture sizes in one launch (kvz_hip_batch_group) ----
 * A batch fixes ONE geometry, and a small batch's pass cannot fill the device: a service with 1080p, 832x480 and 4K streams would run one thin launch per size, or
 * split the workgroup slots by hand (kvz_hip_batch_set_device_share).  A group joins the CTU passes -- the one kernel that needs everybody's parallelism -- of its
 * batches into ONE persistent launch over every CTU of every picture of every batch.  Everything else stays per batch and is used as before: buffers, stream,
 * uploads, downloads, loop filters, entropy coder, hashes, distortion.
 * n >= 1 distinct batches of one device, any geometries (equal ones too), ticket schedule.  Builds the joint ticket lists (WPP and raster) and the device-side
 * records once.  NULL + message: n < 1, a NULL or repeated batch, batches on different devices, a batch under KVZ_HIP_SCHED=wave, 65 536 or more pictures in total.
 * The batches must outlive the group. */
typedef struct kvz_hip_batch_group kvz_hip_batch_group;
kvz_hip_batch_group *kvz_hip_batch_group_create(kvz_hip_batch *const *batches, int n);
void                 kvz_hip_batch_group_destroy(kvz_hip_batch_group *g);
/* One launch over every CTU of every picture of every batch.  models[i] is batch i's table (one model for all of a batch's pictures is a table with n_models == 1).
 * Afterwards every batch is in the state its own kvz_hip_intra_frames_models(batch i, models[i]) would have left it in, byte for byte (reconstruction, levels, CU
 * depths and modes, CTU costs, the border records the coder's row contexts come from), and it is that batch's next pass: the launch starts after whatever each
 * batch's stream held (a pending kvz_hip_batch_upload_all_async included), everything queued on a batch afterwards starts after the joint pass, and the batch's
 * next upload starts when the joint pass has ended.  A batch stays usable alone between joint launches.
 * The launch takes the device's whole occupancy (a batch's kvz_hip_batch_set_device_share is not consulted).  One kernel build serves it: the tables must agree in
 * search_32x32 and no_wpp; coeff_cabac and signhide may differ from picture to picture and from batch to batch.
 * Returns 1, or -1 with a message on stderr and NOTHING queued on any batch for: a table kvz_hip_intra_frames_models would refuse for its batch; a table with rdoq or
 * search_nxn; a batch that has scaling lists; tables that disagree in search_32x32 or no_wpp; a batch that is invalid since a hand-off wait timed out (kvz_hip_batch_reset).
 * A hand-off wait that times out inside the joint pass poisons the launch as it poisons a batch's own: EVERY batch of the group then reports -1 from sync, download and
 * checksums until it is reset; the message names the batch beside the picture and the CTU. */
int   kvz_hip_batch_group_intra_frames(kvz_hip_batch_group *g, const kvz_hip_picture_models *const *models);
/* device time of the joint launch (milliseconds); call after the batches were synced */
float kvz_hip_batch_group_last_kernel_ms(kvz_hip_batch_group *g);

#ifdef __cplusplus
}
#endif
#endif
