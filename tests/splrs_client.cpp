// splrs_client -- a scripted client of include/webrtc_resampler.h for tests/test_splrs_gpu.py.
//
//   splrs_client script samples.i16 out.i16 log.txt
//
// script lines: "R in out type" (Reset), "N in out type" (ResetIfNeeded), "P length max_len" (Push the next
// `length` samples of samples.i16).  Every line's return value goes to log.txt ("P" lines with outLen), a
// Push's output to out.i16.
#include <stdio.h>

#include <vector>

#include "webrtc_resampler.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* sc = fopen(argv[1], "r");
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  FILE* log = fopen(argv[4], "w");
  if (!sc || !in || !out || !log) return 2;
  webrtc::Resampler r;
  int n = 0;
  if (r.Push(0, 0, 0, 0, n) != -1 || r.Insert(0, 0) != -1 || r.Pull(0, 0, n) != -1) return 3;  // before any Reset
  char op;
  int a, b, c;
  while (fscanf(sc, " %c %d %d", &op, &a, &b) == 3) {
    if (op == 'P') {
      std::vector<int16_t> x(a > 0 ? a : 1), y(b > 0 ? b : 1);
      if (fread(x.data(), sizeof(int16_t), a, in) != (size_t)a) return 4;
      int len = -7;
      const int rc = r.Push(x.data(), a, y.data(), b, len);
      fprintf(log, "P %d %d\n", rc, len);
      if (rc == 0) fwrite(y.data(), sizeof(int16_t), len, out);
    } else {
      if (fscanf(sc, "%d", &c) != 1) return 4;
      const webrtc::ResamplerType t = (webrtc::ResamplerType)c;
      fprintf(log, "%c %d\n", op, op == 'R' ? r.Reset(a, b, t) : r.ResetIfNeeded(a, b, t));
    }
  }
  fclose(out);
  fclose(log);
  return 0;
}
