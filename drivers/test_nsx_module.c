/*
 * test_nsx_module.c -- WAV -> fixed-point noise suppressor -> WAV driver in plain C.
 *
 * Restates the NS_FIXED body of the reference's WebRtc_AMP_Port/test_ns_module.cpp over this library's
 * drop-in WebRtcNsx_* entry points (include/asp_nsx.h): the header is copied to the output, the rate
 * comes from it (8 / 16 kHz: one band), policy 1 (moderate), 10 ms frames.
 *
 *   test_nsx_module in.wav out.wav [-q]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asp_nsx.h"
#include "wav_io.h"

int main(int argc, char* argv[]) {
  if (argc < 3) {
    printf("Usage: test_nsx_module in.wav out.wav\n");
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
    printf("Fail to parse wav file\n");
    return -1;
  }
  if (header.format.bits_per_sample != 16 || header.format.channels != 1) {
    printf("Only 16-bit mono input is supported!\n");
    return -1;
  }
  write_header(&header, fw);
  const int fs = (int)header.format.sample_per_sec;
  const int n = fs / 100;
  NsxHandle* handle = NULL;
  if ((fs != 8000 && fs != 16000) || WebRtcNsx_Create(&handle) != 0 || WebRtcNsx_Init(handle, (uint32_t)fs) != 0 ||
      WebRtcNsx_set_policy(handle, 1) != 0) {
    printf("Fail to create the NSX (a HIP device and 8 / 16 kHz are required)\n");
    return -1;
  }
  int16_t* in = (int16_t*)calloc((size_t)n, sizeof(int16_t));
  int16_t* out = (int16_t*)calloc((size_t)n, sizeof(int16_t));
  int32_t frm_cnt = 0;
  while (!feof(fr)) {
    read_samples(in, n, &header, fr);
    const short* ip[1] = {in};
    short* op[1] = {out};
    WebRtcNsx_Process(handle, ip, 1, op);
    write_samples(out, n, &header, fw);
    if (!quiet) printf("Frame #%d\n", frm_cnt);
    frm_cnt++;
  }
  printf("%d frames\n", frm_cnt);
  WebRtcNsx_Free(handle);
  fclose(fr);
  fclose(fw);
  free(in);
  free(out);
  return 0;
}
