/*
 * asp_bt.h -- C-ABI of the MI355X batched time-frequency block-thresholding
 * denoiser (Yu/Mallat/Bacry), the reference's Denoise/BlockThresholding.
 *
 * Layer 1: the reference's own per-stream API, signature-identical
 * (Denoise/BlockThresholding/src/audioDenoiseBlockTreshold.h:46-74).  The
 * header declares blockThreshold_flush_float with a float* buffer (.h:66)
 * while the definition takes int16_t* (.c:648); the header form is exported.
 * Layer 2: AspBtBatch_*, N independent stream-channels per call, one
 * 8-hop macroblock per stream-channel per call.
 *
 * Window sizes: the reference derives win_size = fs/1000*time_win (.c:91) and
 * kiss_fft factors any length.  This build: every even window of 4 .. 2048
 * samples whose half has no prime factor above 32 (20 ms at 16 kHz = 320,
 * 50 ms = 800, 10 / 20 / 40 ms at 48 kHz = 480 / 960 / 1920, ...) through kiss_fft's
 * mixed-radix plan (radix 4, 2, 3, 5 and the generic butterfly), with tuned
 * kernels for 256 and 1024 (BASELINE configs 1 and 3); anything else
 * (longer than 2048 samples, a larger prime) returns MARS_ERROR_PARAMS.
 */
#ifndef ASP_BT_H_
#define ASP_BT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* audioDenoiseBlockTreshold.h:7-11 */
#define MARS_OK 0x00
#define MARS_ERROR_MEMORY 0x01
#define MARS_ERROR_PARAMS 0x02
#define MARS_NEED_MORE_SAMPLES 0x10
#define MARS_CAN_OUTPUT 0x20

#define ASP_BT_NBLK_TIME 8  /* max_nblk_time, .c:107 */
#define ASP_BT_NBLK_FREQ 16 /* max_nblk_freq, .c:108 */

/* ---------------------------------------------------------------- layer 1 */
typedef struct MarsBlockThreshold MarsBlockThreshold_t;

MarsBlockThreshold_t* blockThreshold_init(int32_t time_win, int32_t fs, int32_t* err); /* .h:46 */
int32_t blockThreshold_reset(MarsBlockThreshold_t* handle);                            /* .h:48 */
int32_t blockThreshold_denoise_int16(MarsBlockThreshold_t* handle, int16_t* in, int32_t in_len);
int32_t blockThreshold_denoise_float(MarsBlockThreshold_t* handle, float* in, int32_t in_len);
int32_t blockThreshold_output_int16(MarsBlockThreshold_t* handle, int16_t* out, int32_t out_len);
int32_t blockThreshold_output_float(MarsBlockThreshold_t* handle, float* out, int32_t out_len);
int32_t blockThreshold_flush_int16(MarsBlockThreshold_t* handle, int16_t* out, int32_t out_len);
int32_t blockThreshold_flush_float(MarsBlockThreshold_t* handle, float* out, int32_t out_len);
void blockThreshold_free(MarsBlockThreshold_t* handle);
int32_t blockThreshold_max_output(const MarsBlockThreshold_t* handle);       /* macro_size    */
int32_t blockThreshold_samples_per_time(const MarsBlockThreshold_t* handle); /* half_win_size */

/* ---------------------------------------------------------------- layer 2 */
typedef struct AspBtBatch AspBtBatch;

/* Per-stream carried state between macroblocks (checkpoint / parity tests):
 * the second half of the analysis buffer and the overlap-add tail. */
typedef struct AspBtState {
  int32_t win_size;
  float inbuf_tail[1024]; /* inbuf[half..win), first half_win entries used */
  float out_tail[1024];   /* outbuf[macro..macro+half)                     */
} AspBtState;

int AspBtBatch_Create(AspBtBatch** out, int num_streams, int win_size, int device);
int AspBtBatch_Free(AspBtBatch* b);
int AspBtBatch_Reset(AspBtBatch* b);
/* blockThreshold_reset of ONE stream-channel of a running batch: its two tails are cleared, the others untouched. */
int AspBtBatch_ResetStream(AspBtBatch* b, int stream);
/* `nblocks` consecutive macroblocks (8 hops each) of every stream-channel in one call: in / out
 * [nblocks][num_streams][macro_size] float32.  With 256- and 1024-sample windows the macroblocks of up to 64 steps
 * go into ONE launch (the hand-off build: a stream-channel's input tail is read from the previous macroblock's
 * input, its overlap-add tail is handed on through memory behind a per-stream counter); results are those of
 * nblocks AspBtBatch_Denoise calls, bit for bit.  Overlapping buffers: the call is always what nblocks Denoise calls on
 * in + k * num_streams * macro_size, out + k * num_streams * macro_size (k = 0 .. nblocks - 1, in that order) are.  A
 * Denoise call reads a stream-channel's input ahead of that stream-channel's first output store, so out == in works
 * in place, and so does out a whole number of macroblock slots (num_streams * macro_size) below in; with out above in
 * a later macroblock reads what an earlier one wrote, and any other offset is undefined.  When [in, in + nblocks *
 * num_streams * macro_size) and the same range of out share memory the hand-off build is not used (it reads a
 * macroblock's input tail from the previous macroblock's input); the same holds for AspBtBatch_TimedSteps over its
 * blocks_in_ring slots.  AspBtBatch_SetFlow: -1 default (on; ASP_BT_FLOW=0 in the
 * environment turns the default off), 0 off (one launch per macroblock), 1 on. */
int AspBtBatch_DenoiseBlocks(AspBtBatch* b, const float* in, float* out, int nblocks, int mem);
int AspBtBatch_SetFlow(AspBtBatch* b, int mode);
int AspBtBatch_num_streams(const AspBtBatch* b);
int AspBtBatch_macro_size(const AspBtBatch* b); /* 8 * win_size / 2 samples per call */
/* One macroblock per stream: in/out [num_streams][macro_size] float in [-1, 1]
 * units (the reference's float path, .c:541-575); out lags in by half a
 * window, as in the reference.  mem: 0 host, 1 device (asp_ns.h ASP_MEM_*). */
int AspBtBatch_Denoise(AspBtBatch* b, const float* in, float* out, int mem);
/* blockThreshold_flush_float for every stream with `hops` (0..7) pending hops:
 * in [num_streams][hops*half], out [num_streams][hops*half]; no thresholding
 * is applied to a partial macroblock (.c:648-672).  As in the reference the call
 * consumes the overlap tail (a second flush, or the macroblock the pending hops
 * later complete, starts from a cleared tail) and leaves the input history
 * alone (the pending hops stay pending and are fed again with their macroblock). */
int AspBtBatch_Flush(AspBtBatch* b, const float* in, int hops, float* out, int mem);

/* Macroblocks of SOME stream-channels of the batch: list entry i is stream-channel streams[i], which advances by
 * counts[i] macroblocks (counts == NULL: max_blocks each).  in / out: [max_blocks][n][macro_size] float32, row i =
 * entry i (the slot layout of AspBtBatch_DenoiseBlocks with n in place of num_streams); block k of row i is read and
 * written iff k < counts[i]: the rest of in is never interpreted, the rest of out never written.  Streams not listed,
 * and entries with count 0, are untouched: both tails, bit for bit.  What a server needs whose streams joined at
 * different times: the reference feeds hops of half a window and a macroblock completes every eighth hop, so at one
 * tick an eighth of the streams have a macroblock, a late one has two, most have none.  Results, and the state left
 * behind, are bit for bit those of the lock-step calls fed the same macroblocks per stream.
 *
 * AspBtBatch_FlushList: entry i flushes stream-channel streams[i] with hops[i] (0 .. 7) pending hops (hops == NULL:
 * max_hops each); in / out: [n][max_hops * half], entry i uses the first hops[i] * half floats of its row and the
 * rest of its out row is not written.  Per entry it is exactly AspBtBatch_Flush: no thresholding, the overlap tail
 * is consumed, the input history is left alone.  An entry with hops[i] == 0 still consumes its overlap tail (hops == 0
 * consumes the tail, as AspBtBatch_Flush with hops = 0 does) and writes nothing.  To leave a stream alone, do not list it.
 *
 * Both calls:
 *   - streams / counts / hops are HOST arrays, free for reuse when the call returns (also for ASP_MEM_DEVICE, where
 *     the call stays asynchronous on the batch's stream): the batch keeps its own copy of each call's lists in a ring
 *     of 8 slots (pinned host memory plus device memory, an event per slot).  Up to 8 list calls may be in flight; a
 *     ninth BLOCKS the host until the call 8 before it has finished on the device, then enqueues as usual;
 *   - mem applies to the samples; ASP_MEM_HOST copies in and out, returns when done, and changes only the blocks
 *     below counts[i] of out (FlushList: the floats below hops[i] * half of a row);
 *   - max_blocks may exceed 64: the call is cut into launches of at most 64 macroblocks of each entry, in block order
 *     per entry; n == 0 or max_blocks == 0 is ASP_OK and enqueues nothing.  FlushList: only n == 0 does nothing,
 *     max_hops == 0 with n > 0 still consumes the listed overlap tails (in / out may then be NULL);
 *   - out == in works in place; any other overlap of [in, in + max_blocks * n * macro_size) (FlushList: n * max_hops *
 *     half) with the same range of out is refused;
 *   - refused before anything is enqueued, the batch left as it was, with ASP_ERR_PARAM (the last-error record has
 *     the reason): such an overlap, a null pointer, n outside 0 .. num_streams, a stream outside the batch or listed
 *     twice, a count outside 0 .. max_blocks or hops outside 0 .. max_hops, max_hops outside 0 .. 7, a bad mem;
 *   - every window the batch accepts: 256 and 1024 samples on the tuned kernel (a workgroup walks its entry's
 *     macroblocks itself; at 256 samples four entries per workgroup, each to its own count), the other windows,
 *     every flush, samples that are not 8-byte aligned and ASP_BT_OLD_KERNEL=1 on the plain kernels' list form;
 *   - list calls neither poll nor publish the hand-off counters and AspBtBatch_SetFlow does not affect them:
 *     lock-step Denoise / DenoiseBlocks (hand-off build on or off), ResetStream, Export / ImportState and list calls
 *     interleave freely on one batch, ordered by the batch's stream. */
int AspBtBatch_DenoiseList(AspBtBatch* b, const int32_t* streams, const int32_t* counts, int n, const float* in,
                           float* out, int max_blocks, int mem);
int AspBtBatch_FlushList(AspBtBatch* b, const int32_t* streams, const int32_t* hops, int n, const float* in,
                         float* out, int max_hops, int mem);
int AspBtBatch_ExportState(AspBtBatch* b, int stream, AspBtState* out);
int AspBtBatch_ImportState(AspBtBatch* b, int stream, const AspBtState* in);
int AspBtBatch_Synchronize(AspBtBatch* b);
/* The batch's hipStream_t: device-memory calls are enqueued on it (events around them: tools/bt_list_perf.py). */
void* AspBtBatch_GetStream(AspBtBatch* b);
int AspBtBatch_TimedSteps(AspBtBatch* b, const float* in, float* out, int blocks_in_ring,
                          int steps, float* elapsed_ms);

/* kiss_fftr / kiss_fftri seam for the parity tests (common/kiss_fft/kiss_fftr.c:67-159):
 * forward: time [count][n] -> freq [count][n/2+1] interleaved {r,i};
 * inverse: freq -> time, unscaled.  n in {256, 1024}. */
int AspBt_kiss_fftr_batch(const float* timedata, float* freqdata, int n, int count, int device);
int AspBt_kiss_fftri_batch(const float* freqdata, float* timedata, int n, int count, int device);

#ifdef __cplusplus
}
#endif
#endif /* ASP_BT_H_ */
