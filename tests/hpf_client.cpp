// hpf_client.cpp -- a layer-1 client for the tests: AspHpf_* (include/asp_hpf.h) and webrtc::RMSLevel
// (include/webrtc_rms_level.h) driven from raw int16 files.
//   hpf_client hpf <rate> <n> <in.i16> <out.i16>
//   hpf_client level <channels> <n> <rms_every> <muted_every> <in.i16> <log.txt>
// The meter's schedule is tests/hpf_runs.py's: frame f is ProcessMuted(channels * n) where f % muted_every ==
// muted_every - 1, RMS() follows every rms_every-th frame; the log has one RMS() return per line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "asp_hpf.h"
#include "webrtc_rms_level.h"

static std::vector<int16_t> read_all(const char* path) {
  std::vector<int16_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  int16_t buf[4096];
  size_t got;
  while ((got = fread(buf, sizeof(int16_t), 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "hpf")) {
    const int rate = atoi(argv[2]), n = atoi(argv[3]);
    std::vector<int16_t> x = read_all(argv[4]);
    AspHpf* h = 0;
    if (AspHpf_Create(&h) != 0) return 2;
    if (AspHpf_Process(h, x.data(), n) != ASP_ERR_STATE) return 3;   // before Init
    if (AspHpf_Init(h, 44100) != ASP_ERR_PARAM || AspHpf_Init(h, rate) != 0) return 4;
    for (size_t i = 0; i + n <= x.size(); i += n)
      if (AspHpf_Process(h, x.data() + i, n) != 0) return 5;
    if (AspHpf_Free(h) != 0) return 6;
    FILE* f = fopen(argv[5], "wb");
    if (!f || fwrite(x.data(), sizeof(int16_t), x.size(), f) != x.size()) return 7;
    fclose(f);
    return 0;
  }
  if (argc == 8 && !strcmp(argv[1], "level")) {
    const int channels = atoi(argv[2]), n = atoi(argv[3]), rms_every = atoi(argv[4]), muted_every = atoi(argv[5]);
    std::vector<int16_t> x = read_all(argv[6]);
    FILE* log = fopen(argv[7], "w");
    if (!log) return 7;
    webrtc::RMSLevel level;
    if (!level.ok()) return 2;
    if (level.RMS() != webrtc::RMSLevel::kMinLevel) return 3;
    const size_t frame = (size_t)channels * n;
    for (size_t f = 0; (f + 1) * frame <= x.size(); ++f) {
      if (muted_every && (int)(f % muted_every) == muted_every - 1)
        level.ProcessMuted((int)frame);
      else
        for (int c = 0; c < channels; ++c) level.Process(x.data() + f * frame + (size_t)c * n, n);
      if ((f + 1) % rms_every == 0) fprintf(log, "%d\n", level.RMS());
    }
    level.Process(x.data(), n);
    level.Reset();
    fprintf(log, "%d\n", level.RMS());   // kMinLevel after Reset
    fclose(log);
    return 0;
  }
  fprintf(stderr, "usage: hpf_client hpf|level ...\n");
  return 1;
}
