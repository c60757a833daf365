/*
 * test_aecm_module.c -- WAV -> mobile echo canceller -> WAV driver in plain C.
 *
 * Restates the loop of the reference's WebRtc_AMP_Port/test_aecm_module.cpp over this library's
 * drop-in WebRtcAecm_* entry points (include/asp_aecm.h): the mic header is copied to the output, the
 * rate comes from it, 10 ms frames, msInSndCardBuf 410, nearendClean NULL; per frame BufferFarend on the
 * speaker signal, then Process on the mic signal.
 *
 *   test_aecm_module mic.wav speaker.wav out.wav [-q]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asp_aecm.h"
#include "wav_io.h"

int main(int argc, char* argv[]) {
  if (argc < 4) {
    printf("Usage: test_aecm_module mic.wav speaker.wav out.wav\n");
    return -1;
  }
  const int quiet = argc > 4 && strcmp(argv[4], "-q") == 0;
  FILE* fmic = fopen(argv[1], "rb");
  FILE* fspk = fopen(argv[2], "rb");
  FILE* fout = fopen(argv[3], "wb");
  if (!fmic || !fspk || !fout) {
    printf("Fail to open file !!!\n");
    return -1;
  }
  WAV_HEADER hmic, hspk;
  if (read_header(&hmic, fmic) != 0 || read_header(&hspk, fspk) != 0) {
    printf("Fail to parse wav file\n");
    return -1;
  }
  if (hmic.format.bits_per_sample != 16 || hmic.format.channels != 1) {
    printf("Only 16-bit mono input is supported!\n");
    return -1;
  }
  write_header(&hmic, fout);
  const int fs = (int)hmic.format.sample_per_sec;
  const int n = fs / 100;
  int16_t* mic = (int16_t*)calloc((size_t)n, sizeof(int16_t));
  int16_t* spk = (int16_t*)calloc((size_t)n, sizeof(int16_t));
  int16_t* out = (int16_t*)calloc((size_t)n, sizeof(int16_t));
  void* aecm = NULL;
  if (WebRtcAecm_Create(&aecm) != 0 || WebRtcAecm_Init(aecm, fs) != 0) {
    printf("Fail to create the AECM (a HIP device and 8 / 16 kHz are required)\n");
    return -1;
  }
  int32_t frm_cnt = 0;
  while (!feof(fmic) && !feof(fspk)) {
    read_samples(mic, n, &hmic, fmic);
    read_samples(spk, n, &hspk, fspk);
    WebRtcAecm_BufferFarend(aecm, spk, (int16_t)n);
    WebRtcAecm_Process(aecm, mic, NULL, out, (int16_t)n, 410);
    write_samples(out, n, &hmic, fout);
    if (!quiet) printf("Frame #%d\n", frm_cnt);
    frm_cnt++;
  }
  printf("%d frames\n", frm_cnt);
  WebRtcAecm_Free(aecm);
  fclose(fmic);
  fclose(fspk);
  fclose(fout);
  free(mic);
  free(spk);
  free(out);
  return 0;
}
