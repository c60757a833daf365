/* agc_client.c -- a C client of include/asp_agc.h's layer 1, driven by a script (tests/test_agc_gpu.py):
 *   N                       a new instance (the previous one is freed)
 *   I min max mode fs       WebRtcAgc_Init
 *   C target comp limiter   WebRtcAgc_set_config, then get_config must give the same back
 *   F n                     WebRtcAgc_AddFarend on the next n samples of the input file
 *   M nb n                  WebRtcAgc_AddMic on the next nb * n samples, kept as the current frame
 *   V nb n level            WebRtcAgc_VirtualMic likewise
 *   L nb n                  loads the next nb * n samples as the current frame
 *   P nb n level echo       WebRtcAgc_Process on the current frame; the output goes to the output file
 * Every call's return value (and levels, warning) is one line of the log. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asp_agc.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE *sc = fopen(argv[1], "r"), *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb"), *log = fopen(argv[4], "w");
  if (!sc || !in || !out || !log) return 2;
  void* h = NULL;
  int16_t cur[3][160], res[3][160], far[160];
  int16_t *curp[3] = {cur[0], cur[1], cur[2]}, *resp[3] = {res[0], res[1], res[2]};
  char op;
  int a, b, c, d;
  while (fscanf(sc, " %c", &op) == 1) {
    if (op == 'N') {
      if (h) WebRtcAgc_Free(h);
      if (WebRtcAgc_Create(&h) != 0) return 3;
    } else if (op == 'I') {
      unsigned fs;
      if (fscanf(sc, "%d %d %d %u", &a, &b, &c, &fs) != 4) return 2;
      fprintf(log, "I %d\n", WebRtcAgc_Init(h, a, b, (int16_t)c, fs));
    } else if (op == 'C') {
      if (fscanf(sc, "%d %d %d", &a, &b, &c) != 3) return 2;
      WebRtcAgcConfig cfg = {(int16_t)a, (int16_t)b, (uint8_t)c}, got = {0, 0, 0};
      const int rc = WebRtcAgc_set_config(h, cfg);
      if (WebRtcAgc_get_config(h, &got) != 0 || got.targetLevelDbfs != a || got.compressionGaindB != b || got.limiterEnable != c)
        return 4;
      fprintf(log, "C %d\n", rc);
    } else if (op == 'F') {
      if (fscanf(sc, "%d", &a) != 1 || fread(far, 2, a, in) != (size_t)a) return 2;
      fprintf(log, "F %d\n", WebRtcAgc_AddFarend(h, far, (int16_t)a));
    } else if (op == 'M' || op == 'V' || op == 'L') {
      if (fscanf(sc, "%d %d", &a, &b) != 2) return 2;
      for (int k = 0; k < a; ++k)
        if (fread(cur[k], 2, b, in) != (size_t)b) return 2;
      if (op == 'M') fprintf(log, "M %d\n", WebRtcAgc_AddMic(h, curp, (int16_t)a, (int16_t)b));
      if (op == 'V') {
        int32_t lv = -1;
        if (fscanf(sc, "%d", &c) != 1) return 2;
        const int rc = WebRtcAgc_VirtualMic(h, curp, (int16_t)a, (int16_t)b, c, &lv);
        fprintf(log, "V %d %d\n", rc, lv);
      }
    } else if (op == 'P') {
      if (fscanf(sc, "%d %d %d %d", &a, &b, &c, &d) != 4) return 2;
      int32_t lv = -1;
      uint8_t sat = 9;
      const int rc = WebRtcAgc_Process(h, (const int16_t* const*)curp, (int16_t)a, (int16_t)b, resp, c, &lv, (int16_t)d, &sat);
      fprintf(log, "P %d %d %d\n", rc, lv, sat);
      for (int k = 0; k < a; ++k) fwrite(res[k], 2, b, out);
    } else {
      return 2;
    }
  }
  if (h) WebRtcAgc_Free(h);
  fclose(out);
  fclose(log);
  return 0;
}
