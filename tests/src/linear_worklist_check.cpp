// csrc/linear_worklist.h on the CPU (tests/test_linear_worklist.py builds this with AddressSanitizer + UBSan; no device, nothing
// preloaded): the work list of an all-Linear container's batch for the assignments a host makes — every stream on one size, sizes
// sorted by stream, sizes interleaved (every tile mixed), a lone stream on a size — at 1, 32, 33 and 70 streams. The submodels are the
// fixture's (33, 65, 257 and 1,025 taps: 1 x 64, 1 x 128, 3 x 128, 9 x 128) and the bench's (512, 2,048, 8,192: 4, 16, 64 x 128).
#include <cstdio>
#include <vector>

#include "linear_worklist.h"

using namespace namhip;

static int failures = 0;

#define CHECK(cond)                                                              \
  do                                                                             \
  {                                                                              \
    if (!(cond))                                                                 \
    {                                                                            \
      std::printf("linear_worklist_check: line %d: %s\n", __LINE__, #cond);      \
      failures++;                                                                \
    }                                                                            \
  } while (0)

static std::vector<LinearSub> subs_of(std::initializer_list<std::pair<int, int>> plans)
{
  std::vector<LinearSub> subs;
  int off = 0;
  for (const auto& p : plans)
  {
    LinearSub s;
    s.n_splits = p.first;
    s.split_taps = p.second;
    s.taps_off = off + kLinearPad;
    s.bias = 0.25f * (float)(subs.size() + 1);
    subs.push_back(s);
    off += 2 * kLinearPad + p.first * p.second;
  }
  return subs;
}

// what holds for every assignment
static void check(const std::vector<int>& stream_sub, const std::vector<LinearSub>& subs, int expect_pairs)
{
  const int n = (int)stream_sub.size(), n_subs = (int)subs.size();
  const LinearWorkCaps caps = linear_work_caps(n, subs.data(), n_subs);
  LinearWorkList wl;
  CHECK(build_linear_worklist(stream_sub.data(), n, subs.data(), n_subs, wl));
  CHECK(caps.tiles == (n + 31) / 32 && caps.cols_pad == 32 * caps.tiles && caps.cols_pad >= n);
  CHECK((int)wl.col_pair.size() == caps.cols_pad);
  CHECK(expect_pairs < 0 || (int)wl.pairs.size() == expect_pairs);
  // pairs <= tiles x submodels, and at least one per tile; the grid extents and `part` within what creation allocated
  CHECK((int64_t)wl.pairs.size() <= caps.max_pairs && (int)wl.pairs.size() >= caps.tiles);
  CHECK(wl.grid_splits >= 1 && wl.grid_splits <= caps.max_splits);
  CHECK(wl.part_slabs <= caps.max_part_slabs);
  CHECK(linear_part_floats(wl.part_slabs, 512) <= linear_part_floats(caps.max_part_slabs, 512));
  // every stream's column points at a pair of its own tile and size
  for (int s = 0; s < n; s++)
  {
    const int p = wl.col_pair[(size_t)s];
    CHECK(p >= 0 && p < (int)wl.pairs.size());
    if (p < 0 || p >= (int)wl.pairs.size())
      continue;
    CHECK(wl.pairs[(size_t)p].col_tile == s / 32 && wl.pairs[(size_t)p].sub == stream_sub[(size_t)s]);
  }
  for (int c = n; c < caps.cols_pad; c++) // the padding reduces nothing
    CHECK(wl.col_pair[(size_t)c] == -1);
  // no pair without a stream; the entries are their submodel's; the slabs are disjoint, in order and inside the list's count
  std::vector<int> users(wl.pairs.size(), 0);
  for (int s = 0; s < n; s++)
    if (wl.col_pair[(size_t)s] >= 0 && wl.col_pair[(size_t)s] < (int)users.size())
      users[(size_t)wl.col_pair[(size_t)s]]++;
  int64_t slab = 0;
  int max_splits = 0;
  for (size_t p = 0; p < wl.pairs.size(); p++)
  {
    const LinearPair& e = wl.pairs[p];
    CHECK(users[p] > 0);
    CHECK(e.sub >= 0 && e.sub < n_subs && e.col_tile >= 0 && e.col_tile < caps.tiles);
    if (e.sub < 0 || e.sub >= n_subs)
      continue;
    const LinearSub& u = subs[(size_t)e.sub];
    CHECK(e.n_splits == u.n_splits && e.split_taps == u.split_taps && e.taps_off == u.taps_off && e.bias == u.bias);
    CHECK(e.split_taps <= caps.max_split_taps && e.n_splits * e.split_taps <= caps.max_hist_taps);
    CHECK(e.part_slab == slab);
    slab += e.n_splits;
    max_splits = e.n_splits > max_splits ? e.n_splits : max_splits;
    CHECK(p == 0 || wl.pairs[p - 1].col_tile < e.col_tile || (wl.pairs[p - 1].col_tile == e.col_tile && wl.pairs[p - 1].sub < e.sub));
  }
  CHECK(slab == wl.part_slabs && max_splits == wl.grid_splits);
}

int main()
{
  const std::vector<LinearSub> fixture = subs_of({{1, 64}, {1, 128}, {3, 128}, {9, 128}});
  const std::vector<LinearSub> bench = subs_of({{4, 128}, {16, 128}, {64, 128}});
  for (const std::vector<LinearSub>& subs : {fixture, bench})
  {
    const int W = (int)subs.size();
    {
      const LinearWorkCaps c = linear_work_caps(70, subs.data(), W);
      CHECK(c.tiles == 3 && c.cols_pad == 96 && c.max_pairs == 3 * W);
      CHECK(c.max_splits == subs.back().n_splits && c.max_split_taps == 128 && c.max_hist_taps == subs.back().n_splits * 128);
    }
    for (int n : {1, 32, 33, 70})
    {
      const int tiles = (n + 31) / 32;
      for (int w = 0; w < W; w++) // all streams on one size: one pair per tile
        check(std::vector<int>((size_t)n, w), subs, tiles);
      {
        std::vector<int> sorted((size_t)n), mixed((size_t)n);
        for (int s = 0; s < n; s++)
        {
          sorted[(size_t)s] = (int)((long)s * W / n); // sizes sorted by stream
          mixed[(size_t)s] = s % W; // interleaved: every tile mixed
        }
        check(sorted, subs, -1);
        int expect = 0;
        for (int t = 0; t < tiles; t++)
          expect += (n - 32 * t < 32 ? n - 32 * t : 32) < W ? (n - 32 * t) : W;
        check(mixed, subs, expect);
      }
      for (int lone = 0; lone < n; lone += (n > 8 ? n / 3 : 1)) // a lone stream on a size: one pair more, in its tile
      {
        std::vector<int> a((size_t)n, W - 1);
        a[(size_t)lone] = 0;
        check(a, subs, n == 1 ? 1 : tiles + ((lone / 32 == (n - 1) / 32 && n - 32 * (lone / 32) == 1) ? 0 : 1));
      }
    }
  }
  {
    // the GPU test's assignment: s % 4 for streams 0 - 31, one size for 32 - 63, two sizes among 64 - 69
    std::vector<int> a(70);
    for (int s = 0; s < 70; s++)
      a[(size_t)s] = s < 32 ? s % 4 : s < 64 ? 2 : (s % 2 ? 0 : 3);
    check(a, fixture, 4 + 1 + 2);
    LinearWorkList wl;
    CHECK(build_linear_worklist(a.data(), 70, fixture.data(), 4, wl) && wl.part_slabs == 14 + 3 + 10 && wl.grid_splits == 9);
    a[5] = 4; // no such submodel
    CHECK(!build_linear_worklist(a.data(), 70, fixture.data(), 4, wl));
    a[5] = -1;
    CHECK(!build_linear_worklist(a.data(), 70, fixture.data(), 4, wl));
  }
  if (failures)
    return 1;
  std::printf("linear_worklist_check: ok\n");
  return 0;
}
