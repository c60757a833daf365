// ts_client.cpp -- a client of include/webrtc_transient_suppressor.h for tests/test_ts_gpu.py: reads a script
// (rate, detection rate, channels, chunks, reference length) and per chunk "voice key has_reference", the
// samples from a float32 file, and writes what Suppress left in the data plus one return value per line.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "webrtc_transient_suppressor.h"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  FILE* script = fopen(argv[1], "r");
  FILE* in = fopen(argv[2], "rb");
  FILE* ref_in = fopen(argv[3], "rb");
  FILE* out = fopen(argv[4], "wb");
  FILE* log = fopen(argv[5], "w");
  if (!script || !in || !ref_in || !out || !log) return 2;
  int rate, det_rate, channels, chunks, ref_len;
  if (fscanf(script, "%d %d %d %d %d", &rate, &det_rate, &channels, &chunks, &ref_len) != 5) return 2;
  webrtc::TransientSuppressor ts;
  fprintf(log, "%d\n", ts.Initialize(rate + 1, det_rate, channels));
  fprintf(log, "%d\n", ts.Initialize(rate, det_rate, channels));
  const size_t len = rate / 100;
  std::vector<float> x(len * channels), ref(ref_len);
  for (int f = 0; f < chunks; ++f) {
    float voice;
    int key, has_ref;
    if (fscanf(script, "%f %d %d", &voice, &key, &has_ref) != 3) return 2;
    if (fread(x.data(), sizeof(float), x.size(), in) != x.size()) return 2;
    if (fread(ref.data(), sizeof(float), ref.size(), ref_in) != ref.size()) return 2;
    fprintf(log, "%d\n", ts.Suppress(x.data(), len, channels, NULL, det_rate / 100, has_ref ? ref.data() : NULL,
                                      ref.size(), voice, key != 0));
    fwrite(x.data(), sizeof(float), x.size(), out);
  }
  fprintf(log, "%d\n", ts.Suppress(x.data(), len + 1, channels, NULL, det_rate / 100, NULL, 0, 0.5f, false));
  fclose(out);
  fclose(log);
  return 0;
}
