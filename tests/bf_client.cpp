// bf_client.cpp -- a client of include/webrtc_beamformer.h for tests/test_bf_abi.py (compiles) and
// tests/test_bf_gpu.py (runs): arguments are the microphone count, the spacing in metres, the chunk count,
// whether the high band is passed, and four files.  Reads [chunks][mics][160] float32 per band, writes the
// low-band output (processed in place: output[0] is input[0]) and the high-band output, and logs status() and
// is_target_present() per chunk.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "webrtc_beamformer.h"

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  const int mics = atoi(argv[1]), chunks = atoi(argv[3]), with_high = atoi(argv[4]);
  const float spacing = (float)atof(argv[2]);
  FILE* in = fopen(argv[5], "rb");
  FILE* high_in = fopen(argv[6], "rb");
  FILE* out = fopen(argv[7], "wb");
  FILE* high_out = fopen(argv[8], "wb");
  FILE* log = fopen(argv[9], "w");
  if (!in || !high_in || !out || !high_out || !log) return 2;
  std::vector<webrtc::Point> geometry;
  for (int c = 0; c < mics; ++c) geometry.push_back(webrtc::Point(c * spacing, 0.f, 0.f));
  webrtc::Beamformer bf(geometry);
  bf.Initialize(10, 8000);  // refused: the status says so and the object stays usable
  fprintf(log, "%d\n", bf.status());
  bf.Initialize(10, 16000);
  fprintf(log, "%d\n", bf.status());
  const size_t n = 160;
  std::vector<float> x(n * mics), hi(n * mics), hy(n);
  std::vector<float*> xp(mics), hp(mics);
  for (int c = 0; c < mics; ++c) {
    xp[c] = &x[c * n];
    hp[c] = &hi[c * n];
  }
  float* hyp[1] = {&hy[0]};
  for (int f = 0; f < chunks; ++f) {
    if (fread(&x[0], sizeof(float), x.size(), in) != x.size()) return 2;
    if (fread(&hi[0], sizeof(float), hi.size(), high_in) != hi.size()) return 2;
    bf.ProcessChunk(&xp[0], with_high ? &hp[0] : NULL, mics, (int)n, &xp[0], hyp);
    fprintf(log, "%d %d\n", bf.status(), bf.is_target_present() ? 1 : 0);
    fwrite(xp[0], sizeof(float), n, out);
    if (with_high) fwrite(&hy[0], sizeof(float), n, high_out);
  }
  bf.ProcessChunk(&xp[0], NULL, mics + 1, (int)n, &xp[0], hyp);  // the reference CHECKs here
  fprintf(log, "%d\n", bf.status());
  fclose(out);
  fclose(high_out);
  fclose(log);
  return 0;
}
