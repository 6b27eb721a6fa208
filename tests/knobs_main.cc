// Host-only probe of csrc/knobs.h for tests/test_knobs_cpu.py: prints what one accessor of each read kind returns under the
// environment the test started it with, one "NAME=value" line each.  Built with the host compiler alone (no HIP).
#include <cstdio>
#include "knobs.h"

namespace k = aocr::knob;

static void show(const char* name, bool v) { std::printf("%s=%d\n", name, v ? 1 : 0); }
static void show(const char* name, int v) { std::printf("%s=%d\n", name, v); }
static void show(const char* name, const char* v) { if (v) std::printf("%s=[%s]\n", name, v); else std::printf("%s=null\n", name); }

int main() {
  show("SET", k::AOCR_HALO8());
  show("ON", k::AOCR_NO_DMA());
  show("NOT0", k::AOCR_WGRAD_HALO_RAGGED());
  show("INT", k::AOCR_HALO4_STAGED());
  show("RAW", k::AOCR_ENC_BWD_RH());
  show("MINK", k::AOCR_F32W_MINK());
  show("CUS", k::AOCR_COMM_RESERVE_CUS());
  show("STOP", k::AOCR_DBG_STOP());
  show("STOP_SET", k::AOCR_DBG_STOP_SET());
  // every accessor reads the environment on every call: a change made by this process is seen by the next call
  const bool before = k::AOCR_NO_QUARTER_TILES();
  setenv("AOCR_NO_QUARTER_TILES", "1", 1);
  const bool set = k::AOCR_NO_QUARTER_TILES();
  unsetenv("AOCR_NO_QUARTER_TILES");
  std::printf("REREAD=%d%d%d\n", before ? 1 : 0, set ? 1 : 0, k::AOCR_NO_QUARTER_TILES() ? 1 : 0);
  return 0;
}
