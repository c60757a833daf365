/*
 * test_vad_module.c -- WAV -> voice activity detector -> WAV driver in plain C.
 *
 * Restates the loop of the reference's WebRtc_AMP_Port/test_vad_module.cpp over this library's
 * drop-in WebRtcVad_* entry points (include/asp_vad.h): header copied verbatim, 10 ms frames
 * (length = fs / 100), mode 2 (aggressive), and per frame +16383 for speech, -16383 for no speech and
 * 0 when WebRtcVad_Process fails.  The `while (!feof)` loop also processes the final short read with
 * the stale tail of the previous frame, as drivers/test_ns_module.c does.
 *
 *   test_vad_module mic.wav vad_result.wav [-q]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asp_vad.h"
#include "wav_io.h"

int main(int argc, char* argv[]) {
  if (argc < 3) {
    printf("Usage: test_vad_module mic.wav vad_result.wav\n");
    return -1;
  }
  const int quiet = argc > 3 && strcmp(argv[3], "-q") == 0;
  FILE* fr = fopen(argv[1], "rb");
  FILE* fw = fopen(argv[2], "wb");
  if (!fr || !fw) {
    printf("Fail to open file !!!\n");
    return -1;
  }
  WAV_HEADER header;
  if (read_header(&header, fr) != 0) {
    printf("Fail to parse wav file: %s\n", argv[1]);
    return -1;
  }
  if (header.format.bits_per_sample != 16) {
    printf("Now only support 16 bits per sample!\n");
    return -1;
  }
  if (header.format.channels != 1) {
    printf("Only mono input is supported!\n");
    return -1;
  }
  write_header(&header, fw);
  const int fs = (int)header.format.sample_per_sec;
  const int length = fs / 100;
  int16_t* mic = (int16_t*)calloc((size_t)length, sizeof(int16_t));
  int16_t* result = (int16_t*)calloc((size_t)length, sizeof(int16_t));
  VadInst* vad = NULL;
  if (WebRtcVad_Create(&vad) != 0 || WebRtcVad_Init(vad) != 0 || WebRtcVad_set_mode(vad, 2) != 0) {
    printf("Fail to create the VAD (a HIP device is required)\n");
    return -1;
  }
  int32_t frm_cnt = 0;
  while (!feof(fr)) {
    read_samples(mic, length, &header, fr);
    const int r = WebRtcVad_Process(vad, fs, mic, length);
    const int16_t v = r == 1 ? 16383 : (r == 0 ? -16383 : 0);
    for (int i = 0; i < length; ++i) result[i] = v;
    write_samples(result, length, &header, fw);
    if (!quiet) printf("Frame #%d\n", frm_cnt);
    frm_cnt++;
  }
  printf("%d frames\n", frm_cnt);
  WebRtcVad_Free(vad);
  fclose(fr);
  fclose(fw);
  free(mic);
  free(result);
  return 0;
}
