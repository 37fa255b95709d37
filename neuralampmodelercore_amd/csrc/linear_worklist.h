// linear_worklist.h — the work list of a SlimmableContainer of Linear models: which (column tile, submodel) pairs
// one launch piece computes, which pair every column's output comes from, how far the grid extends and how many partial sums it
// writes. A plain function of the streams' assignment and the submodels' split plans. Host only, no HIP header, so
// tests/src/linear_worklist_check.cpp walks it on the CPU. api_launch.cpp (the batch's tables) and kernel_linear.hip (the entry
// type) are the users.
#pragma once

#include <cstdint>
#include <vector>

#include "plan.h"

namespace namhip
{
// One submodel as a pair needs it: its K-splits (LinearPlan), where its lag 0 sits in the batch's blob (the submodels' blobs behind
// one another), its bias.
struct LinearSub
{
  int32_t n_splits = 1, split_taps = kBlock, taps_off = 0;
  float bias = 0.0f;
};

// A device table entry: the streams of column tile `col_tile` (32 columns, column = stream) that run submodel `sub`. The pair's
// partial sums are slabs [part_slab, part_slab + n_splits) of `part` = [slab][frame][32].
struct LinearPair
{
  int32_t col_tile, sub, taps_off, split_taps, n_splits, part_slab;
  float bias;
  int32_t reserved;
};
static_assert(sizeof(LinearPair) == 32, "kernel_linear.hip reads the table as 32-byte records");

// What a batch allocates at creation: the worst assignment (every tile runs every submodel)
struct LinearWorkCaps
{
  int32_t tiles = 0, cols_pad = 0;
  int64_t max_pairs = 0; // tiles x submodels
  int32_t max_splits = 0, max_split_taps = 0; // the largest over the submodels: the grid's split extent, the dynamic LDS
  int32_t max_hist_taps = 0; // the largest n_splits x split_taps: the ring keeps that many frames + one launch piece
  int64_t max_part_slabs = 0; // tiles x the sum of the submodels' n_splits
};
inline LinearWorkCaps linear_work_caps(int n_streams, const LinearSub* subs, int n_subs)
{
  LinearWorkCaps c;
  c.tiles = (n_streams + kLinearColTile - 1) / kLinearColTile;
  c.cols_pad = c.tiles * kLinearColTile;
  c.max_pairs = (int64_t)c.tiles * n_subs;
  int64_t splits = 0;
  for (int i = 0; i < n_subs; i++)
  {
    c.max_splits = subs[i].n_splits > c.max_splits ? subs[i].n_splits : c.max_splits;
    c.max_split_taps = subs[i].split_taps > c.max_split_taps ? subs[i].split_taps : c.max_split_taps;
    const int32_t taps = subs[i].n_splits * subs[i].split_taps;
    c.max_hist_taps = taps > c.max_hist_taps ? taps : c.max_hist_taps;
    splits += subs[i].n_splits;
  }
  c.max_part_slabs = (int64_t)c.tiles * splits;
  return c;
}

struct LinearWorkList
{
  std::vector<LinearPair> pairs; // by tile, then by submodel
  std::vector<int32_t> col_pair; // [cols_pad]: the pair a column's output is reduced from; -1 for the padding behind n_streams
  int32_t grid_splits = 0; // the largest n_splits among `pairs`
  int64_t part_slabs = 0; // slabs the pairs write
};
inline int64_t linear_part_floats(int64_t slabs, int part_frames)
{
  return slabs * part_frames * kLinearColTile;
}

// stream_sub[s] = the submodel stream s runs. False (and `out` unspecified) when an entry names no submodel.
inline bool build_linear_worklist(const int* stream_sub, int n_streams, const LinearSub* subs, int n_subs, LinearWorkList& out)
{
  const LinearWorkCaps caps = linear_work_caps(n_streams, subs, n_subs);
  out.pairs.clear();
  out.col_pair.assign((size_t)caps.cols_pad, -1);
  out.grid_splits = 0;
  out.part_slabs = 0;
  std::vector<int32_t> pair_of_sub((size_t)n_subs);
  for (int t = 0; t < caps.tiles; t++)
  {
    const int s0 = t * kLinearColTile, s1 = s0 + kLinearColTile < n_streams ? s0 + kLinearColTile : n_streams;
    pair_of_sub.assign((size_t)n_subs, -1);
    for (int s = s0; s < s1; s++)
    {
      if (stream_sub[s] < 0 || stream_sub[s] >= n_subs)
        return false;
      pair_of_sub[(size_t)stream_sub[s]] = 0; // in use
    }
    for (int w = 0; w < n_subs; w++)
    {
      if (pair_of_sub[(size_t)w] < 0)
        continue;
      pair_of_sub[(size_t)w] = (int32_t)out.pairs.size();
      LinearPair p;
      p.col_tile = t;
      p.sub = w;
      p.taps_off = subs[w].taps_off;
      p.split_taps = subs[w].split_taps;
      p.n_splits = subs[w].n_splits;
      p.part_slab = (int32_t)out.part_slabs;
      p.bias = subs[w].bias;
      p.reserved = 0;
      out.pairs.push_back(p);
      out.part_slabs += p.n_splits;
      out.grid_splits = p.n_splits > out.grid_splits ? p.n_splits : out.grid_splits;
    }
    for (int s = s0; s < s1; s++)
      out.col_pair[(size_t)s] = pair_of_sub[(size_t)stream_sub[s]];
  }
  return true;
}

} // namespace namhip
