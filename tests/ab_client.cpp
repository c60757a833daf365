// ab_client.cpp -- a C++ client of include/asp_audio_buffer.h for the tests: compiles against the header alone and
// links against the library.
//   ab_client identity <streams> <in.i16> <out.i16>
// 16 kHz mono frames of 160 samples, <streams> at a time: DeinterleaveFrom, the float view, the rounded int16 view,
// InterleaveTo; the output equals the input.  Without arguments it prints the usage; the refusals that need no device
// are checked on the way.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "asp_audio_buffer.h"

int main(int argc, char** argv) {
  AspAudioBufferBatch* b = 0;
  // refused before a device is looked at
  if (AspAudioBufferBatch_Create(&b, 1, 160, 3, 160, 1, 160, 0) != ASP_ERR_PARAM || b) return 10;
  if (AspAudioBufferBatch_Create(&b, 1, 160, 1, 160, 2, 160, 0) != ASP_ERR_PARAM || b) return 11;
  if (AspAudioBufferBatch_Create(&b, 1, 100, 1, 160, 1, 160, 0) != ASP_ERR_PARAM || b) return 12;
  if (!strstr(AspNs_last_error(), "samples")) return 13;
  if (argc == 5 && !strcmp(argv[1], "identity")) {
    const int S = atoi(argv[2]);
    std::vector<int16_t> x;
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 2;
    int16_t buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(int16_t), 4096, f)) > 0) x.insert(x.end(), buf, buf + got);
    fclose(f);
    if (AspAudioBufferBatch_Create(&b, S, 160, 1, 160, 1, 160, 0) != ASP_OK) return 3;
    const size_t frame = (size_t)S * 160;
    std::vector<int32_t> act(S, ASP_AB_VAD_ACTIVE), back(S, -1);
    for (size_t i = 0; i + frame <= x.size(); i += frame) {
      if (AspAudioBufferBatch_DeinterleaveFrom(b, x.data() + i, act.data(), ASP_MEM_HOST) != ASP_OK) return 4;
      if (!AspAudioBufferBatch_channels_f(b) || !AspAudioBufferBatch_channels_const(b)) return 5;
      if (AspAudioBufferBatch_split_channels_const(b, 1) || AspAudioBufferBatch_low_pass_reference(b)) return 6;
      if (AspAudioBufferBatch_InterleaveTo(b, x.data() + i, back.data(), 1, ASP_MEM_HOST) != ASP_OK) return 7;
      if (back[S - 1] != ASP_AB_VAD_ACTIVE) return 8;
    }
    if (AspAudioBufferBatch_Free(b) != ASP_OK) return 9;
    f = fopen(argv[4], "wb");
    if (!f || fwrite(x.data(), sizeof(int16_t), x.size(), f) != x.size()) return 2;
    fclose(f);
    return 0;
  }
  fprintf(stderr, "usage: ab_client identity <streams> <in.i16> <out.i16>\n");
  return 1;
}
