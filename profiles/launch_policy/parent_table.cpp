// The stage choice of launch_wr at the parent commit: its two lambdas copied verbatim (api_launch.cpp:305-371), with parameters in
// place of the batch's fields (b->n_cus, b->wr_max_stages), `ok` in place of wr_jit_function's answer and `gate` for line 310.
#include <algorithm>
#include <cstdio>

#include "plan.h"

using namespace namhip;

struct Shape
{
  int stages, lds_bytes;
  bool dense;
};

static Shape parent(int total, int lds_bytes, int n_cus, int wr_max_stages, bool can_split, bool can_split4, int ok, bool gate)
{
  int stages = 1;
  bool dense = false;
  if (gate)
  {
    const int cus = std::max(n_cus, 1);
    auto duration = [&](int nst) {
      const int lds = lds_bytes + (nst - 1) * kWrQueueBytes;
      if (lds > kWrMaxLdsBytes)
        return 1e9;
      const int on_chip = cus * std::min(4 / nst, (160 * 1024) / (lds + 512));
      const double speed = nst == 4 ? 3.1 : nst == 2 ? 1.75 : 1.0;
      const int turns = (total + on_chip - 1) / on_chip;
      return turns * (1.0 + 0.15 * (turns - 1)) / speed; // a turn's last workgroups leave SIMDs idle; images move in and out
    };
    double best = duration(1);
    if (can_split && wr_max_stages >= 2 && duration(2) < 0.9 * best)
    {
      stages = 2;
      best = duration(2);
    }
    if (can_split && can_split4 && wr_max_stages >= 4 && duration(4) < 0.9 * best)
    {
      stages = 4;
      best = duration(4);
    }
    const bool plain_fills = ((long)total * stages) % (4l * cus) == 0;
    if (can_split && wr_max_stages >= 2 && !plain_fills)
    {
      if (ok != 0)
      {
        auto duration_dense = [&](int nst) {
          const int lds = lds_bytes + (nst - 1) * kWrQueueBytes;
          if (lds > kWrMaxLdsBytes)
            return 1e9;
          const int on_chip = cus * std::min(8 / nst, (160 * 1024) / (lds + 512));
          const double speed = 0.9 * (nst == 4 ? 3.1 : 1.75);
          const int turns = (total + on_chip - 1) / on_chip;
          return turns * (1.0 + 0.15 * (turns - 1)) / speed;
        };
        if ((ok & 2) && duration_dense(2) < 0.9 * best)
        {
          stages = 2;
          dense = true;
          best = duration_dense(2);
        }
        if ((ok & 4) && can_split4 && wr_max_stages >= 4 && duration_dense(4) < 0.9 * best)
        {
          stages = 4;
          dense = true;
        }
      }
    }
    lds_bytes += (stages - 1) * kWrQueueBytes;
  }
  return {stages, lds_bytes, dense};
}

static void row(int lds, int ok, std::initializer_list<int> totals, int cus = 256, int max_stages = 4, bool cs = true, bool cs4 = true)
{
  std::printf("lds %6d bits %d cus %3d max %d split %d%d:", lds, ok, cus, max_stages, (int)cs, (int)cs4);
  for (int t : totals)
  {
    const Shape s = parent(t, lds, cus, max_stages, cs, cs4, ok, true);
    std::printf(" %d->%d%s", t, s.stages, s.dense ? "d" : "");
  }
  std::printf("\n");
}

// one answer for every stream count 1 .. 4,096 and every set of dense forms, or "varies"
static void every(int lds)
{
  const Shape first = parent(1, lds, 256, 4, true, true, 0, true);
  bool same = true;
  for (int ok = 0; ok <= 6; ok += 2)
    for (int t = 1; t <= 4096; t++)
    {
      const Shape s = parent(t, lds, 256, 4, true, true, ok, true);
      same = same && s.stages == first.stages && !s.dense;
    }
  std::printf("lds %6d bits any, 1 .. 4096 streams: %s %d\n", lds, same ? "always" : "varies, first", first.stages);
}

int main()
{
  std::printf("kWrQueueBytes %d kWrMaxLdsBytes %d\n", kWrQueueBytes, kWrMaxLdsBytes);
  row(8192, 0, {1, 256, 257, 512, 513, 1024});
  row(8192, 6, {256, 257, 512, 513, 768, 1024, 1025, 2048, 2049});
  row(39936, 6, {768, 769, 1024, 1025, 1537, 2049, 2305, 2561});
  row(53248, 0, {256, 257, 513, 769, 1024, 1025, 1537, 2049});
  row(53248, 6, {256, 257, 513, 769, 1024, 1025, 1537, 2049});
  row(73264, 0, {12, 1536, 1792, 1793, 2049});
  row(73264, 6, {12, 1536, 1792, 1793, 2049});
  every(133120);
  every(153600);
  row(8192, 0, {1, 64}, 8);
  row(8192, 6, {257}, 8);
  row(8192, 0, {256}, 256, 2);
  row(8192, 0, {256}, 256, 4, true, false);
  row(8192, 6, {256}, 256, 4, false, true);
  row(8192, 2, {768});
  row(8192, 4, {768});
  row(8192, 0, {768}, 0);
  const Shape s = parent(12, 73264, 256, 4, true, true, 6, true), off = parent(12, 73264, 256, 4, true, true, 6, false);
  std::printf("lds 73264, 12 streams: %d stages, %d bytes; gate off: %d stage(s), %d bytes\n", s.stages, s.lds_bytes, off.stages, off.lds_bytes);
  return 0;
}
