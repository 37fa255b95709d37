// csrc/launch_policy.h on the CPU (tests/test_launch_resident.py builds this with AddressSanitizer + UBSan; no device, nothing
// preloaded): launch_all_resident / wr_all_resident — are all workgroups of a session's launch on the chip at once? Only such a
// launch may linger for its next command (csrc/persist_wave.h: wait_command); one that runs in turns publishes and leaves. The
// values at the documented bounds, monotone in the workgroup count, and the same answer as the rules that were there before
// (wr_stream_bound, wr_duration's turns, wr_launch_shape) wherever they speak about the same thing.
#include <cstdio>

#include "launch_policy.h"

using namespace namhip;
using namespace namhip::api;

static int failures = 0;

#define CHECK(cond)                                                             \
  do                                                                            \
  {                                                                             \
    if (!(cond))                                                                \
    {                                                                           \
      std::printf("launch_resident_check: line %d: %s\n", __LINE__, #cond);     \
      failures++;                                                               \
    }                                                                           \
  } while (0)

static WrShapeQuery query(int lds, int bits, int total, int cus, bool multi)
{
  WrShapeQuery q;
  q.total = total;
  q.lds_bytes = lds;
  q.cus = cus;
  q.max_stages = 4;
  q.can_split = q.can_split4 = true;
  q.dense_forms = bits;
  q.multi_buffer = multi;
  return q;
}

int main()
{
  // the plain rule at its boundaries: n_wg <= per_cu x CUs; nothing fits where nothing is asked for or nothing fits a CU; 0 CUs count as 1
  CHECK(launch_all_resident(1, 1, 1) && !launch_all_resident(2, 1, 1));
  CHECK(launch_all_resident(1024, 4, 256) && !launch_all_resident(1025, 4, 256));
  CHECK(launch_all_resident(256, 1, 256) && !launch_all_resident(257, 1, 256));
  CHECK(!launch_all_resident(0, 4, 256) && !launch_all_resident(-1, 4, 256) && !launch_all_resident(1, 0, 256));
  CHECK(launch_all_resident(4, 4, 0) && !launch_all_resident(5, 4, 0));
  CHECK(launch_all_resident(0x7fffffff, 0x7fffffff, 0x7fffffff)); // (no overflow: the product is taken in 64 bits)
  // monotone in n_wg: once a launch no longer fits, no larger one does
  for (int per_cu = 1; per_cu <= 8; per_cu++)
    for (int cus : {1, 8, 256, 304})
    {
      bool fits = true;
      int last = 0;
      for (int n = 1; n <= per_cu * cus + 64; n++)
      {
        const bool f = launch_all_resident(n, per_cu, cus);
        CHECK(fits || !f);
        if (f)
          last = n;
        fits = f;
      }
      CHECK(last == per_cu * cus);
    }

  // the LSTM kernels: one wavefront per SIMD whatever the instantiation's registers — 4 workgroups per CU. The row kernel holds four
  // streams per workgroup: 4,096 streams on 256 CUs linger, 4,100 (1,025 workgroups) take turns; persist_kind admits 8 per CU
  CHECK(kLstmRowResidentPerCu == 4 && kLstmWideResidentPerCu == 4);
  CHECK(launch_all_resident((4096 + 3) / 4, kLstmRowResidentPerCu, 256) && !launch_all_resident((4097 + 3) / 4, kLstmRowResidentPerCu, 256));
  CHECK(launch_all_resident((13 + 3) / 4, kLstmRowResidentPerCu, 256)); // (thirteen streams: four workgroups, the last one holds one stream)
  CHECK(launch_all_resident(1024, kLstmWideResidentPerCu, 256) && !launch_all_resident(1025, kLstmWideResidentPerCu, 256));
  CHECK(!launch_all_resident(8 * 256, kLstmRowResidentPerCu, 256)); // (what persist_kind still admits as a session: in turns)

  // nam_wn_reg_kernel, one wavefront per stream: exactly one turn's share of wr_stream_bound (= kPersistTurns turns) fits at once
  for (int lds : {0, 8192, 40448, 40449, 54101, 54102, 73264, 81408, 81409, kWrMaxLdsBytes})
    for (int cus : {0, 1, 8, 256})
    {
      const int turn = wr_stream_bound(lds, cus) / kPersistTurns;
      CHECK(wr_stream_bound(lds, cus) == turn * kPersistTurns);
      CHECK(launch_all_resident(turn, wr_workgroups_per_cu(lds, 1, 1), cus));
      CHECK(!launch_all_resident(turn + 1, wr_workgroups_per_cu(lds, 1, 1), cus));
      // a one-buffer launch is one wavefront per stream: wr_all_resident asks the same
      const WrShapeQuery q1 = query(lds, 0, turn, cus, false), q2 = query(lds, 0, turn + 1, cus, false);
      CHECK(wr_all_resident(q1, wr_launch_shape(q1)) && !wr_all_resident(q2, wr_launch_shape(q2)));
    }

  // ... and in the form wr_launch_shape chooses: resident exactly when wr_duration counts ONE turn for that form
  for (int lds : {8192, 39936, 53248, 73264, 133120, 153600})
    for (int bits : {0, 6})
      for (int cus : {8, 256})
      {
        for (int total = 1; total <= 5 * 4 * cus; total += (cus == 256 ? 7 : 1))
        {
          const WrShapeQuery q = query(lds, bits, total, cus, true);
          const WrLaunchShape s = wr_launch_shape(q);
          const int per_simd = s.dense ? 2 : 1;
          const int on_chip = cus * wr_workgroups_per_cu(s.lds_bytes, s.stages, per_simd);
          const bool f = wr_all_resident(q, s);
          CHECK(f == ((total + on_chip - 1) / on_chip == 1));
          // a launch that fits is never slower, by the cost model, than a turn of one-wave workgroups is long
          if (f)
            CHECK(wr_duration(q, s.stages, per_simd) <= 1.0);
          // whatever form is chosen, a launch beyond what the chip holds as one wavefront per SIMD of one-wave workgroups never fits
          if (total > 4 * per_simd * cus)
            CHECK(!f);
        }
      }
  // the record of the nano model (73,264 bytes) on 256 CUs: twelve streams run four wavefronts each and fit; 256 streams as four
  // wavefronts fill the chip (one workgroup per CU) and fit; 1,793 streams run one wave each, two per CU (512 at once): turns
  {
    WrShapeQuery q = query(73264, 0, 12, 256, true);
    CHECK(wr_launch_shape(q).stages == 4 && wr_all_resident(q, wr_launch_shape(q)));
    q.total = 256;
    CHECK(wr_launch_shape(q).stages == 4 && wr_all_resident(q, wr_launch_shape(q)));
    q.total = 257;
    CHECK(wr_launch_shape(q).stages == 4 && !wr_all_resident(q, wr_launch_shape(q)));
    q.total = 1793;
    CHECK(wr_launch_shape(q).stages == 1 && !wr_all_resident(q, wr_launch_shape(q)));
    q.total = 512;
    q.multi_buffer = false;
    CHECK(wr_all_resident(q, wr_launch_shape(q)));
    q.total = 513;
    CHECK(!wr_all_resident(q, wr_launch_shape(q)));
  }

  if (failures)
    return 1;
  std::printf("launch_resident_check: ok\n");
  return 0;
}
