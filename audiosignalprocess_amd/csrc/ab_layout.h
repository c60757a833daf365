// ab_layout.h -- what the audio buffer's kernels (ab_kernels.hip) and host code (ab_api.hip) agree on: the device
// storage of a batch, the kernels' argument blocks, and the checkpoint blob.
//
// Device storage, S streams, Cp processing channels, U = S * Cp stream-channels, P processing samples, nb bands of
// ns = 160 samples (nb = 1, ns = P on a buffer without bands):
//   ch_i   int16 [U][P]        ch_f   float [U][P]          channels_  (IFChannelBuffer: the int16 / float pair)
//   band_i int16 [nb][U][ns]   band_f float [nb][U][ns]     split_channels_ (AspSplitBatch's band layout)
//   mixed  int16 [S][ns]                                     mixed_low_pass_channels_
//   ref    int16 [U][ns]                                     low_pass_reference_channels_
//   rs_in  float [U][Pin + 32] rs_out float [U][P + 32]      the resamplers' input buffers (SincResampler)
// [U][n] is [S][Cp][n]: the layout the other batches take with one frame and C = Cp.
#ifndef ASP_AB_LAYOUT_H_
#define ASP_AB_LAYOUT_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_audio_buffer.h"
#include "sinc_layout.h"
#include "sinc_plan.h"

namespace aspab {

constexpr int kBandSamples = 160;   // kSamplesPer16kHzChannel
constexpr int kGroup = 4;           // samples a lane of an element-wise kernel moves: 8 bytes of int16, 16 of float
constexpr int kElemBlock = 256;

// ---- element-wise kernels.  A work item is (stream, group of kGroup consecutive samples); consecutive lanes take
// consecutive groups of a stream's row, so every access of a wave is a run of whole 8- or 16-byte pieces.

struct InterleaveArgs {
  int16_t* ch_i;         // [S][Cp][n]
  const float* ch_f;     // InterleaveTo with a stale int16 side: read here, FloatS16ToS16, and refresh ch_i
  int16_t* frames;       // [S][n * Cin]
  int S, n, Cin, Cp;
  int from_float;
};

// RefreshI over a set of buffers laid out [nb][S][Cp][ns], optionally with the two consumers of band 0
struct RefreshIArgs {
  int16_t* bi;
  const float* bf;
  int16_t* mixed;        // non-null: (a + b) / 2 of band 0's two channels -> [S][ns]
  int16_t* ref;          // non-null: band 0 -> [S][Cp][ns]
  int S, Cp, ns, nb;
  int mask;              // bit k: band k is refreshed from its float side
};

struct RefreshFArgs {
  const int16_t* src;
  float* dst;
  int groups;            // elements / kGroup
};

// ---- resampling kernels: one workgroup per stream-channel
struct CopyArgs {
  float* state;                  // [U][buf_len] or null without a resampler
  const float* ktable;           // [33 * 32]
  const aspsinc::OutDesc* desc;  // the call's descriptors; channel c's start at desc_off[c]
  aspsinc::SincPlan plan[2];     // per processing channel (the output resamplers of two channels may differ in position)
  int desc_off[2];
  int buf_len, src_frames, dst_frames;
  int S, Cp, Cin, Cio;           // Cio: channels of the caller's array per stream (CopyFrom: Cin + keyboard; CopyTo: num_channels)
  const float* in_f;             // CopyFrom: caller's [S][Cio][src_frames];  CopyTo: ch_f
  const int16_t* in_i;           // CopyTo with a stale float side: ch_i (and ch_f is refreshed)
  float* out;                    // CopyFrom: ch_f [U][dst_frames];  CopyTo: caller's [S][Cio][dst_frames]
  float* refresh_f;              // CopyTo from ch_i: ch_f
};

// ---- checkpoint
struct AbRecord {
  int32_t magic;                 // kRecordMagic
  int32_t geometry[5];           // input_samples, Cin, proc_samples, Cp, output_samples
  int32_t num_channels;
  int32_t ch_ivalid, ch_fvalid, band_ivalid[ASP_AB_MAX_BANDS], band_fvalid[ASP_AB_MAX_BANDS];
  int32_t mixed_valid, reference_copied;
  int32_t reserved;
  aspsinc::SincPos in_pos, out_pos[2];
};
constexpr int32_t kRecordMagic = 0x41423031;   // "AB01"
static_assert(sizeof(AbRecord) % 8 == 0, "the resampler buffers follow the record");

}  // namespace aspab

#endif  // ASP_AB_LAYOUT_H_
