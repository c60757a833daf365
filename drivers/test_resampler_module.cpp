// test_resampler_module -- the reference's resampler driver (WebRtc_AMP_Port/test_resampler_module.cpp)
// restated over include/webrtc_resampler.h: a 16-bit WAV file through webrtc::Resampler, 10 ms per Push.
//
//   test_resampler_module in_file out_file out_rate
//
// As in the reference, the output header is the input's with sample_per_sec replaced, a Push's return value
// is not looked at, and write_samples gets whatever out_len holds (after a rejected Push: the previous
// frame's count, and the previous frame's samples).  Two departures: the reference takes the input rate
// from the header after it has overwritten it with out_rate, so it only ever copies; this driver reads it
// before.  And the output buffer holds 12 x the input frame (the largest ratio, 1To12), where the
// reference's 4 x makes Push reject 8 -> 44.1 and 8 -> 48 kHz.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "webrtc_resampler.h"
extern "C" {
#include "wav_io.h"
}

using namespace webrtc;

int main(int argc, char* argv[]) {
  if (argc < 4) {
    printf("Usage: %s in_file out_file out_rate\n", argv[0]);
    return -1;
  }
  printf("Process %s -> %s\n", argv[1], argv[2]);
  FILE* fr = fopen(argv[1], "rb");
  FILE* fw = fopen(argv[2], "wb");
  if (!fr || !fw) {
    printf("Can't open file!\n");
    return -1;
  }
  WAV_HEADER header;
  if (read_header(&header, fr) != 0) {
    printf("Fail to read wav header!\n");
    return -1;
  }
  print_header(&header);
  const uint32_t frequency = header.format.sample_per_sec;
  header.format.sample_per_sec = atoi(argv[3]);
  write_header(&header, fw);
  if (header.format.bits_per_sample != 16) {
    printf("Now only support 16 bits per sample!\n");
    return -1;
  }
  const uint16_t length = frequency / 100;

  Resampler resampler(frequency, atoi(argv[3]), kResamplerSynchronous);

  int16_t* input = new int16_t[length];
  int16_t* output = new int16_t[12 * length];
  memset(input, 0, length * sizeof(int16_t));
  memset(output, 0, 12 * length * sizeof(int16_t));

  int32_t frm_cnt = 0;
  int out_len = 0;
  while (!feof(fr)) {
    read_samples(input, length, &header, fr);
    resampler.Push(input, length, output, 12 * length, out_len);
    write_samples(output, out_len, &header, fw);
    printf("Frame #%d\n", frm_cnt++);
  }
  fclose(fr);
  fclose(fw);
  delete[] input;
  delete[] output;
  return 0;
}
