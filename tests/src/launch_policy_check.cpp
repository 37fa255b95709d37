// csrc/launch_policy.h on the CPU (tests/test_launch_policy.py builds this with AddressSanitizer + UBSan; no device, nothing
// preloaded): nam_wn_reg_kernel's wavefronts per stream at every stream count where the answer changes. The table is a record of the
// code BEFORE the rule was extracted — launch_wr's two lambdas run with parameters in place of batch fields
// (profiles/launch_policy/README.md) — and its 73,264-byte rows are the GPU record of the nano model
// (profiles/bank_wn_reg/forms_by_stream_count.txt).
#include <cstdio>
#include <initializer_list>

#include "launch_policy.h"

using namespace namhip;
using namespace namhip::api;

static int failures = 0;

#define CHECK(cond)                                                             \
  do                                                                            \
  {                                                                             \
    if (!(cond))                                                                \
    {                                                                           \
      std::printf("launch_policy_check: line %d: %s\n", __LINE__, #cond);       \
      failures++;                                                               \
    }                                                                           \
  } while (0)

static WrShapeQuery base(int lds, int bits, int total)
{
  WrShapeQuery q;
  q.total = total;
  q.lds_bytes = lds;
  q.cus = 256;
  q.max_stages = 4;
  q.can_split = q.can_split4 = true;
  q.dense_forms = bits;
  q.multi_buffer = true;
  return q;
}

// the expected answer, and what holds for every query
static void expect(const WrShapeQuery& q, int stages, bool dense)
{
  const WrLaunchShape s = wr_launch_shape(q);
  if (s.stages != stages || s.dense != dense)
  {
    std::printf("launch_policy_check: lds %d bits %d cus %d max %d split %d%d, %d streams: %d%s, expected %d%s\n", q.lds_bytes, q.dense_forms,
                q.cus, q.max_stages, (int)q.can_split, (int)q.can_split4, q.total, s.stages, s.dense ? "d" : "", stages, dense ? "d" : "");
    failures++;
  }
  CHECK(s.lds_bytes == q.lds_bytes + (s.stages - 1) * kWrQueueBytes);
  CHECK(s.lds_bytes <= kWrMaxLdsBytes);
  CHECK(s.stages <= q.max_stages);
  if (s.dense)
  {
    CHECK(q.dense_forms & s.stages); // (bit 1: two stages, bit 2: four)
    WrShapeQuery plain = q;
    plain.dense_forms = 0;
    CHECK(((long)q.total * wr_launch_shape(plain).stages) % (4l * std::max(q.cus, 1)) != 0);
  }
  WrShapeQuery one = q;
  one.multi_buffer = false;
  const WrLaunchShape o = wr_launch_shape(one);
  CHECK(o.stages == 1 && !o.dense && o.lds_bytes == q.lds_bytes);
}

struct At
{
  int total, stages;
  bool dense;
};
static constexpr bool d = true;

static void rows(int lds, std::initializer_list<int> bits, std::initializer_list<At> at)
{
  for (int b : bits)
    for (const At& a : at)
      expect(base(lds, b, a.total), a.stages, a.dense);
}

int main()
{
  CHECK(kWrQueueBytes == 10304 && kWrMaxLdsBytes == 156 * 1024 && kCuLdsBytes == 160 * 1024);
  // 256 CUs, wr_max_stages 4, both cuts, a multi-buffer launch
  rows(8192, {0}, {{1, 4}, {256, 4}, {257, 2}, {512, 2}, {513, 1}, {1024, 1}});
  rows(8192, {6}, {{256, 4}, {257, 4, d}, {512, 2}, {513, 2, d}, {768, 2, d}, {1024, 1}, {1025, 2, d}, {2048, 1}, {2049, 2, d}});
  rows(39936, {6}, {{768, 2, d}, {769, 4, d}, {1024, 1}, {1025, 2, d}, {1537, 1}, {2049, 2, d}, {2305, 4, d}, {2561, 1}});
  rows(53248, {0, 6}, {{256, 4}, {257, 2}, {513, 1}, {769, 2}, {1024, 2}, {1025, 1}, {1537, 2}, {2049, 1}});
  rows(73264, {0, 6}, {{12, 4}, {1536, 4}, {1792, 4}, {1793, 1}, {2049, 4}});
  CHECK(wr_launch_shape(base(73264, 0, 12)).lds_bytes == 104176);
  for (int b = 0; b <= 6; b += 2)
    for (int t = 1; t <= 4096; t++)
    {
      expect(base(133120, b, t), 2, false); // (four stages' queues no longer fit)
      expect(base(153600, b, t), 1, false); // (nor two stages')
    }
  // the further cases
  WrShapeQuery q = base(8192, 0, 1);
  q.cus = 8;
  expect(q, 4, false);
  q.total = 64;
  expect(q, 1, false);
  q = base(8192, 6, 257);
  q.cus = 8;
  expect(q, 2, d);
  q = base(8192, 0, 256);
  q.max_stages = 2;
  expect(q, 2, false);
  q = base(8192, 0, 256);
  q.can_split4 = false;
  expect(q, 2, false);
  q = base(8192, 6, 256);
  q.can_split = false;
  expect(q, 1, false);
  expect(base(8192, 2, 768), 2, d);
  expect(base(8192, 4, 768), 4, d);
  q = base(8192, 0, 768);
  q.cus = 0; // counted as 1
  expect(q, 1, false);

  // occupancy: four one-wave workgroups per CU while their LDS fits, two two-wave ones, one four-wave one; twice that at two
  // wavefronts per SIMD; and the LDS bound at its boundaries: n workgroups fit up to 163,840 / n - 512 bytes each
  CHECK(wr_workgroups_per_cu(8192, 1, 1) == 4 && wr_workgroups_per_cu(8192, 2, 1) == 2 && wr_workgroups_per_cu(8192, 4, 1) == 1);
  CHECK(wr_workgroups_per_cu(8192, 2, 2) == 4 && wr_workgroups_per_cu(8192, 4, 2) == 2);
  CHECK(wr_workgroups_per_cu(40448, 1, 1) == 4 && wr_workgroups_per_cu(40449, 1, 1) == 3);
  CHECK(wr_workgroups_per_cu(54101, 1, 1) == 3 && wr_workgroups_per_cu(54102, 1, 1) == 2);
  CHECK(wr_workgroups_per_cu(81408, 1, 1) == 2 && wr_workgroups_per_cu(81409, 1, 1) == 1);
  CHECK(wr_workgroups_per_cu(kWrMaxLdsBytes, 1, 1) == 1); // (the planner's limit: one always fits)
  // the stream bound: kPersistTurns x per CU x CUs
  CHECK(wr_stream_bound(8192, 256) == 8192 && wr_stream_bound(73264, 256) == 4096 && wr_stream_bound(kWrMaxLdsBytes, 256) == 2048);
  CHECK(wr_stream_bound(8192, 0) == 32 && wr_stream_bound(0, 8) == 256);

  if (failures)
    return 1;
  std::printf("launch_policy_check: ok\n");
  return 0;
}
