/*
 * asp_ns.h -- C-ABI of the MI355X batched noise-suppression engine.
 *
 * Two layers, both plain C (no C++/torch types cross this boundary):
 *
 *  1. The reference's own per-stream "process-frame" API, signature-identical,
 *     so the unmodified driver logic of WebRtc_AMP_Port/test_ns_module.cpp:59-113
 *     links against this library instead of the reference's C objects:
 *       WebRtcNs_Create / _Free / _Init / _set_policy / _Analyze / _Process /
 *       _prior_speech_probability
 *     (replaces webrtc/modules/audio_processing/ns/include/noise_suppression.h:16-123,
 *      implemented in the reference by ns/noise_suppression.c:20-66 over ns/ns_core.c).
 *     Each handle is a batch of one stream on the GPU.
 *
 *  2. The batched extension AspNsBatch_*: the same verbs with N independent
 *     streams per call, frames laid out [stream][160] float (float-S16 range,
 *     webrtc/modules/audio_processing/audio_buffer.h:71-72), caller-owned,
 *     host or device pointers.  One opaque handle owns all device state.
 *
 * Only fs = 16000 (blockLen 160, anaLen 256, magnLen 129; ns_core.c:93-98) and
 * num_bands = 1 are implemented; other rates return -1 from Init.
 */
#ifndef ASP_NS_H_
#define ASP_NS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASP_NS_BLOCKL 160   /* ns/defines.h:14 */
#define ASP_NS_ANAL 256     /* ns/defines.h:15 */
#define ASP_NS_BINS 129     /* ns/defines.h:16 */
#define ASP_NS_SIMULT 3     /* ns/defines.h:21 */
#define ASP_NS_HIST 1000    /* ns/defines.h:45 */

/* ---------------------------------------------------------------- layer 1 */

typedef struct NsHandleT NsHandle; /* noise_suppression.h:16 */

int WebRtcNs_Create(NsHandle** NS_inst);               /* noise_suppression.h:35  */
int WebRtcNs_Free(NsHandle* NS_inst);                  /* noise_suppression.h:48  */
int WebRtcNs_Init(NsHandle* NS_inst, uint32_t fs);     /* noise_suppression.h:65  */
int WebRtcNs_set_policy(NsHandle* NS_inst, int mode);  /* noise_suppression.h:80  */
void WebRtcNs_Analyze(NsHandle* NS_inst, const float* spframe); /* :93 */
void WebRtcNs_Process(NsHandle* NS_inst,               /* noise_suppression.h:108 */
                      const float* const* spframe,
                      int num_bands,
                      float* const* outframe);
float WebRtcNs_prior_speech_probability(NsHandle* handle); /* :123 */

/* ---------------------------------------------------------------- layer 2 */

/* Canonical, natural-bin-order snapshot of one stream's state.  Field names
 * and meanings follow NoiseSuppressionC (ns/ns_core.h:52-114); it is the
 * checkpoint/restore blob and the teacher-forcing device of the parity tests.
 * speechProb[] is transient on the device (only the >16 kHz high-band branch
 * ns_core.c:1362-1414 reads it across calls) and is exported as zeros. */
typedef struct AspNsState {
  int32_t fs;
  int32_t aggrMode;
  int32_t initFlag;
  int32_t gainmap;
  int32_t blockInd;
  int32_t updates;
  int32_t counter[ASP_NS_SIMULT];
  int32_t modelUpdatePars[4];
  float overdrive;
  float denoiseBound;
  float priorSpeechProb;
  float signalEnergy;
  float sumMagn;
  float whiteNoiseLevel;
  float pinkNoiseNumerator;
  float pinkNoiseExp;
  float priorModelPars[7];
  float featureData[7];
  float analyzeBuf[ASP_NS_ANAL];
  float dataBuf[ASP_NS_ANAL];
  float syntBuf[ASP_NS_ANAL];
  float density[ASP_NS_SIMULT * ASP_NS_BINS];
  float lquantile[ASP_NS_SIMULT * ASP_NS_BINS];
  float quantile[ASP_NS_BINS];
  float smooth[ASP_NS_BINS];
  float noise[ASP_NS_BINS];
  float noisePrev[ASP_NS_BINS];
  float magnPrevAnalyze[ASP_NS_BINS];
  float magnPrevProcess[ASP_NS_BINS];
  float logLrtTimeAvg[ASP_NS_BINS];
  float magnAvgPause[ASP_NS_BINS];
  float initMagnEst[ASP_NS_BINS];
  float parametricNoise[ASP_NS_BINS];
  float speechProb[ASP_NS_BINS];
  int32_t histLrt[ASP_NS_HIST];
  int32_t histSpecFlat[ASP_NS_HIST];
  int32_t histSpecDiff[ASP_NS_HIST];
} AspNsState;

/* High-band analysis buffers of one stream (dataBufHB, ns_core.h:112): only used above 16 kHz,
 * where the band split hands WebRtcNs_Process one or two high bands (ns_core.c:1227-1235,
 * 1362-1414).  Kept apart from AspNsState so that 16 kHz checkpoints do not carry them. */
typedef struct AspNsHbState {
  float dataBufHB[2][ASP_NS_ANAL];
} AspNsHbState;

typedef struct AspNsBatch AspNsBatch;

/* Where the caller's frame buffers live. */
enum { ASP_MEM_HOST = 0, ASP_MEM_DEVICE = 1 };

/* Error codes (layer 2 returns 0 on success, a negative code otherwise). */
enum {
  ASP_OK = 0,
  ASP_ERR_PARAM = -1,    /* bad argument (same value the reference returns)   */
  ASP_ERR_NO_DEVICE = -2,/* no usable HIP device / kernel image not loadable  */
  ASP_ERR_HIP = -3,      /* a HIP call failed (AspNs_last_error has the text,
                            whichever module of the library failed)          */
  ASP_ERR_STATE = -4     /* handle not initialised                            */
};

/* Creates a batch of `num_streams` independent streams on HIP device `device`
 * (sharding hint: one batch per GPU, streams are never exchanged). */
int AspNsBatch_Create(AspNsBatch** out, int num_streams, int device);
int AspNsBatch_Free(AspNsBatch* b);
/* WebRtcNs_Init for every stream (ns_core.c:74-214): fs = 8000 (frames of 80 samples, 128-sample
 * window, 65 bins), 16000, or 32000 / 48000 (the 0-8 kHz band of the band split plus 1 / 2 high
 * bands); frames are 160 samples per stream except at 8000. */
int AspNsBatch_Init(AspNsBatch* b, uint32_t fs);
/* WebRtcNs_set_policy for every stream (ns_core.c:1013-1041). */
int AspNsBatch_set_policy(AspNsBatch* b, int mode);
/* Per-stream control of a running batch, as the reference's per-handle calls give it (noise_suppression.c:35-44):
 * InitStream = WebRtcNs_Init of ONE stream at the batch's sample rate (state and histograms back to InitCore's values,
 * policy 0 as InitCore leaves it), set_policy_stream = WebRtcNs_set_policy of ONE stream.  The other streams are
 * untouched; the calls are ordered on the batch's stream with the frame steps around them. */
int AspNsBatch_InitStream(AspNsBatch* b, int stream);
int AspNsBatch_set_policy_stream(AspNsBatch* b, int stream, int mode);
int AspNsBatch_num_streams(const AspNsBatch* b);

/* frames: [num_streams][160] float ([num_streams][80] at 8 kHz, here and below).  Asynchronous on the batch's HIP stream
 * for ASP_MEM_DEVICE; ASP_MEM_HOST copies in/out and returns when done. */
int AspNsBatch_Analyze(AspNsBatch* b, const float* frames, int mem);
int AspNsBatch_Process(AspNsBatch* b, const float* in, float* out, int mem);
/* Analyze(frame) immediately followed by Process(frame) on the same frame for
 * every stream -- the loop body of test_ns_module.cpp:97-99 -- as one fused
 * launch per frame.  in/out: [num_frames][num_streams][160]; in == out is
 * allowed (the driver aliases them, test_ns_module.cpp:98-99). */
int AspNsBatch_AnalyzeProcess(AspNsBatch* b, const float* in, float* out,
                              int num_frames, int mem);

/* 32 / 48 kHz (AspNsBatch_Init(b, 32000 | 48000)): the band split (asp_split.h) hands the suppressor
 * the 0-8 kHz band plus num_bands - 1 high bands; the low band is processed as above, the high bands
 * get the time-domain gain of ns_core.c:1362-1414.  low [num_frames][num_streams][160],
 * high [num_frames][num_bands - 1][num_streams][160]; in-place (out == in) allowed.
 * AnalyzeProcessBands = WebRtcNs_Analyze(low) + WebRtcNs_Process(bands) per frame
 * (libapm/src/apm_ns.cpp:69-74); ProcessBands = WebRtcNs_Process(bands) after a separate Analyze. */
int AspNsBatch_num_bands(const AspNsBatch* b);
int AspNsBatch_AnalyzeProcessBands(AspNsBatch* b, const float* low_in, const float* high_in,
                                   float* low_out, float* high_out, int num_frames, int mem);
int AspNsBatch_ProcessBands(AspNsBatch* b, const float* low_in, const float* high_in, float* low_out,
                            float* high_out, int mem);
int AspNsBatch_ExportHbState(AspNsBatch* b, int stream, AspNsHbState* out);
int AspNsBatch_ImportHbState(AspNsBatch* b, int stream, const AspNsHbState* in);

/* The same fused step on int16 PCM frames, [num_frames][num_streams][160] int16: what the
 * WAV drivers move (test_ns_module.cpp:85-106).  int16 -> float-S16 on load is value
 * preserving (channel_buffer.cc:43-53); the store applies FloatS16ToS16 rounding
 * (audio_util.h:41-49).  Halves the frame bytes crossing HBM / PCIe. */
int AspNsBatch_AnalyzeProcessS16(AspNsBatch* b, const int16_t* in, int16_t* out,
                                 int num_frames, int mem);

/* Fused Analyze+Process of SOME streams of the batch: list entry i is stream streams[i], which advances by
 * counts[i] frames (counts == NULL: max_frames each).  in / out: [max_frames][n][160], row i = entry i;
 * frame f of row i is used iff f < counts[i]; the rest of out is not written; in == out allowed.
 * Streams not listed, and entries with count 0, are untouched: state, histograms, everything.
 * What a jitter buffer needs: at one tick some streams have no frame, most have one, some a burst of two or three.
 * Results are bit for bit those of the lock-step calls fed the same frames per stream.
 *   - streams / counts are HOST arrays, free for reuse when the call returns (also for ASP_MEM_DEVICE, where the call
 *     stays asynchronous on the batch's stream: the batch keeps its own copy of each call's lists, in a ring of 8
 *     slots.  Up to 8 list calls may be in flight; a further call BLOCKS the host until the call 8 before it has
 *     finished on the device, then enqueues as usual);
 *   - mem applies to the frames; ASP_MEM_HOST copies in and out, returns when done, and changes only rows and frames
 *     below counts[i] of out;
 *   - max_frames may exceed 64: the call is cut into launches of at most 64 frames of each entry, in stream order;
 *     n == 0 or max_frames == 0 is ASP_OK and enqueues nothing;
 *   - refused before anything is enqueued, the batch left as it was (AspNs_last_error has the reason):
 *     ASP_ERR_PARAM for a null pointer, n outside 0 .. num_streams, a stream outside the batch or listed twice, a
 *     count outside 0 .. max_frames, a bad mem; ASP_ERR_STATE for a batch that is not initialised or not at 16 kHz
 *     (this is the one-band 16 kHz geometry: no 8 kHz, no 32 / 48 kHz bands), after SetKernel 1 or 2 (their sums
 *     associate differently), after a two-call Analyze / Process (unpaired streams), or while a diagnostic of the
 *     pair-layout kernel (step counts, timeline, stamps) is on;
 *   - there is one form: SetFlow, SetFlowWalk, SetSplit and SetGraph do not affect it (SetSteady does), and it
 *     leaves the hand-off build's step counters alone, so lock-step calls go on before and after. */
int AspNsBatch_AnalyzeProcessList(AspNsBatch* b, const int32_t* streams, const int32_t* counts, int n,
                                  const float* in, float* out, int max_frames, int mem);
int AspNsBatch_AnalyzeProcessListS16(AspNsBatch* b, const int32_t* streams, const int32_t* counts, int n,
                                     const int16_t* in, int16_t* out, int max_frames, int mem);

int AspNsBatch_ExportState(AspNsBatch* b, int stream, AspNsState* out);
int AspNsBatch_ImportState(AspNsBatch* b, int stream, const AspNsState* in);
/* priorSpeechProb of every stream (noise_suppression.c:57-66), out[num_streams]. */
int AspNsBatch_prior_speech_probability(AspNsBatch* b, float* out);

/* Launch stream control: by default the batch owns a private HIP stream.
 * SetStream adopts a caller-owned hipStream_t (passed as void*). */
int AspNsBatch_SetStream(AspNsBatch* b, void* hip_stream);
/* Issue the fused step of a large batch as `parts` (1..4) independent
 * sub-launches on separate HIP streams (streams never interact, so results are
 * unchanged); lets one part's memory phases overlap another part's arithmetic. */
int AspNsBatch_SetSplit(AspNsBatch* b, int parts);
/* Which fused-step kernel serves AnalyzeProcess: 0 / 3 (default) = one stream per wave64 in the pair
 * layout (two bins per lane, ns_kernels1.hip), 1 = one stream per wave64 with bins q / q + 64
 * (ns_kernels.hip, the kernel of the two-call Analyze / Process protocol).  Same arithmetic; the ~10
 * cross-bin sums per frame are associated differently, so outputs agree to reduction-order rounding. */
int AspNsBatch_SetKernel(AspNsBatch* b, int kernel);
/* Hand-off build of the multi-frame entry points (AnalyzeProcess / AnalyzeProcessS16 with num_frames >= 2,
 * AnalyzeProcessReplay, TimedSteps) on the pair-layout kernel: up to 64 consecutive frame steps of a call go
 * into ONE launch (grid y = step), and a per-stream step counter in device memory orders step k + 1 of a
 * stream behind its own step k (every state access write-through / L1-bypassing), so consecutive steps overlap
 * on the chip instead of meeting at a launch boundary.  Same arithmetic, same results bit for bit; every step
 * still reads and writes the whole state through memory (nothing of a stream stays on chip between steps).
 * mode: -1 = default (on; the environment variable ASP_NS_FLOW=0 turns the default off), 0 = off, 1 = on.
 * A wait that times out (workgroups are dispatched in grid order, so it cannot) makes the next synchronising
 * call fail with ASP_ERR_HIP. */
int AspNsBatch_SetFlow(AspNsBatch* b, int mode);
/* Hand-off build, pair-layout kernel: how many consecutive frame steps of a launch one workgroup walks for its four
 * streams (tables, barrier and lane set-up once per walk; only the walk's first step waits for a counter).
 * 0 = auto, sized to the launch: 8 steps when the batch has at least one workgroup (four streams) per compute unit
 * of its device -- ceil(num_streams / 4) >= hipDeviceProp_t::multiProcessorCount, 1024 streams on an MI355X -- and 4
 * steps for a smaller batch; a launch shorter than that is one walk.  The rule looks at nothing else (why 8, and why
 * that boundary: the comment above flow_walk_auto in csrc/ns_api.hip).  1..64 force a length (the environment variable
 * ASP_NS_FLOW_WALK does the same for batches left on auto).  Same results bit for bit for every value. */
int AspNsBatch_SetFlowWalk(AspNsBatch* b, int steps);
/* Pair-layout kernel: a frame step of a stream in steady state -- past both start-up windows, no quantile tracker
 * publishing, the feature-histogram window staying open, gain compensation on: all but a few steps in 200 of a
 * long-running stream -- takes a body compiled under those conditions, every other step the generic one; one
 * wave-uniform predicate chooses per step.  Same arithmetic, same results bit for bit.  on: -1 = default (on; the
 * environment variable ASP_NS_STEADY=0 turns the default off), 0 = off (every step through the generic body: A / B
 * runs and tests), 1 = on. */
int AspNsBatch_SetSteady(AspNsBatch* b, int on);
/* Test hook: on != 0 makes the batch's pair-layout launches (float frames) run the diagnostic kernels, which add up,
 * per stream, the frame steps that took the steady body and the generic one; counts ([num_streams][2], host, may be
 * NULL) receives the sums so far.  on == 0 reads them a last time and returns to the product kernels.  While it is on,
 * an int16 call (AnalyzeProcessS16) is refused with ASP_ERR_STATE: the diagnostic kernels take float frames. */
int AspNsBatch_DebugStepCounts(AspNsBatch* b, int on, unsigned* counts);
/* Test hook: the grid's y extent (chunks of steps = ceil(steps / walk)) of the batch's last hand-off launch of the
 * pair-layout kernel; 0 before the first one. */
int AspNsBatch_DebugFlowChunks(AspNsBatch* b, int* chunks);
/* Test hook: puts the host's hand-off step counter one ahead of the device's, so that the next multi-frame
 * call's waits time out (about 0.2 s), its steps are skipped and the call (or the next synchronising one)
 * returns ASP_ERR_HIP; the counters are back in step afterwards and the batch needs AspNsBatch_Init. */
int AspNsBatch_DebugFlowDesync(AspNsBatch* b);
void* AspNsBatch_GetStream(AspNsBatch* b);
int AspNsBatch_Synchronize(AspNsBatch* b);

/* The box's streaming-copy rate: a float4 copy of `bytes` bytes repeated `iters` times on
 * `device`, *gbps = (bytes read + bytes written) / hipEvent time, best of three timed passes.
 * bench.py prints it as roofline.copy_ceiling next to the 8 TB/s HBM spec peak. */
int AspNs_CopyCeiling(size_t bytes, int iters, int device, double* gbps);

/* Device scratch for callers without their own allocator (C drivers, bench). */
int AspNs_DeviceAlloc(void** ptr, size_t bytes, int device);
int AspNs_DeviceFree(void* ptr);
int AspNs_MemcpyH2D(void* dst, const void* src, size_t bytes);
int AspNs_MemcpyD2H(void* dst, const void* src, size_t bytes);

/* `steps` fused frame steps on device buffers in/out ([frames_in_ring][num_streams][160], step k
 * uses ring slot k % frames_in_ring), enqueued asynchronously as ONE replay of a captured hipGraph
 * (kernel nodes only, one launch per frame step and sub-launch, exactly the launches
 * AspNsBatch_AnalyzeProcess would issue).  The capture is cached while the arguments stay the
 * same, so a caller that feeds the same ring repeatedly pays one graph launch per call.
 * Replay must be enabled with AspNsBatch_SetGraph(b, 1); it is off by default (plain launches measured
 * faster), and with it off this call enqueues the same launches one by one. */
int AspNsBatch_AnalyzeProcessReplay(AspNsBatch* b, const float* in, float* out,
                                    int frames_in_ring, int steps);
int AspNsBatch_SetGraph(AspNsBatch* b, int on);

/* Timed replay for bench.py: runs `steps` fused frame-steps on device buffers
 * in/out ([frames_in_ring][num_streams][160], step k uses ring slot k %
 * frames_in_ring) on the batch's stream, bracketed by hipEvents recorded on
 * that stream.  *elapsed_ms receives the event time for all steps. */
int AspNsBatch_TimedSteps(AspNsBatch* b, const float* in, float* out,
                          int frames_in_ring, int steps, float* elapsed_ms);
/* Host time (microseconds) the last AspNsBatch_TimedSteps call spent enqueuing its launches. */
int AspNsBatch_LastEnqueueUs(AspNsBatch* b, double* us);

/* Number of HIP devices visible, or a negative error code. */
int AspNs_device_count(void);
/* Compute units of HIP device `device` (hipDeviceProp_t::multiProcessorCount): what AspNsBatch_SetFlowWalk's
 * automatic length is sized by. */
int AspNs_device_compute_units(int device, int* compute_units);
/* Text of the most recent failure on this thread ("" if none).  The record is library-wide: a failure
   of any module (NS, BT, AEC, split, resample, VAD, AECM, NSX) overwrites it. */
const char* AspNs_last_error(void);

/* Host copy of the constant tables the kernels use (layout: struct NsTables in
 * audiosignalprocess_amd/csrc/ns_layout.h); needs no device. */
int AspNs_host_tables(void* out, size_t bytes);
size_t AspNs_host_tables_size(void);

/* Test seams for the device math.  fn: 0 = the kernels' (float)log((double)x)
 * (lean fp64 path with libm fallback), 1/2/3 = libm-based (float)log / exp /
 * tanh of (double)x; 4 = x / param, 5 = the kernels' division by a wave-uniform
 * divisor, 6 = the kernels' lean division x / param, 7 = param / x, 8 = lean
 * param / x, 9 = sqrtf, 10 = the kernels' sqrt, 11 / 12 = the kernels' exp / tanh;
 * 23 = the pair-layout frame step's form of the tanh (debug_compare only, as fn_a
 * beside fn_b = 3).
 * debug_eval maps a host array in place; debug_compare
 * evaluates fn_a and fn_b on every float with bit pattern in
 * [start, start+count) and reports how many differ (first 64 patterns). */
int AspNs_debug_eval(int fn, float* data, size_t n, int device);
int AspNs_debug_compare(int fn_a, int fn_b, uint32_t start, uint32_t count,
                        uint32_t* n_bad, uint32_t* bad_bits64, float param, int device);

/* FFT seam used by the parity tests: batched 256-point real FFT in Ooura
 * packing (a[0]=R0, a[1]=R128, a[2k]=Rk, a[2k+1]=Ik; fft4g.c:90-118), i.e.
 * what WebRtc_rdft(256, isgn, a, ip, w) (fft4g.c:324-362) does to each row.
 * data: [count][256] float, in place; isgn = +1 forward, -1 inverse (unscaled). */
int AspNs_rdft256_batch(float* data, int count, int isgn, int mem, int device);
/* The same seam for WebRtc_rdft(128, isgn), the transform of the 8 kHz geometry: data [count][128]. */
int AspNs_rdft128_batch(float* data, int count, int isgn, int mem, int device);

#ifdef __cplusplus
}
#endif
#endif /* ASP_NS_H_ */
