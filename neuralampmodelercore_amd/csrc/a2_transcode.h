// a2_transcode.h — a narrow A2 container submodel (A2-Lite) between its two residences in a batch: nam_wn_reg_kernel's state
// (STATE_WN_REG: [64 write positions][per layer ceil(C / 4) groups of [R][gs]], plan.h: WrPlan) and the rings of the container's
// largest submodel's layout ([64 write positions][ring r = [R_r][C_full], frame-major]), where a zero-padded copy
// of the submodel runs on nam_kq_kernel next to the Full streams of a mixed persistent session (api_session.cpp: persist_kind).
// Both layouts keep the same quantities: per conv layer the layer's INPUT over the last (K - 1) * dilation + 64 frames, for the head
// rechannel with taps the head accumulator over its (K_h - 1) * dilation + 64 frames, and per ring the index the next frame goes to
// (kernel_wn_reg.hip: "wrap(position - o + j)"; kernel_kq.hip: fetch / "the buffer that starts at write position"). A ring row i
// of one layout is therefore ring row i of the other and the position carries over as it is: the table below names, per ring, where
// each channel's row 0 lies on either side. Host only, no HIP header: tests/src/a2_transcode_check.cpp walks it on the CPU;
// kernel_a2_transcode.hip reads the records, api_launch.cpp builds and uploads them.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "plan.h"

namespace namhip
{
constexpr int kA2XcMaxCh = 16; // channels of a ring of the padded layout (the A1 kernels' limit)

// One ring. Row i (0 <= i < R) of channel c: padded side, float a2_off + i * a2_ch + c of the stream's state; narrow side, float
// wr_off[c] + i * wr_gs[c] for c < wr_ch (channels wr_ch .. a2_ch - 1 exist on the padded side only and are zero there). The
// write positions: int `ring_id` of the padded state, int `slot` of the narrow one.
struct A2XcRing
{
  int32_t R, slot, ring_id, a2_off, a2_ch, wr_ch;
  int32_t wr_off[kA2XcMaxCh], wr_gs[kA2XcMaxCh];
  int32_t reserved[2];
};
static_assert(sizeof(A2XcRing) == 160, "kernel_a2_transcode.hip reads the table as 160-byte records");

struct A2Transcode
{
  bool ok = false;
  std::string why; // !ok: the first thing that does not match
  std::vector<A2XcRing> rings;
  int32_t wr_state_floats = 0, a2_state_floats = 0; // what either side's rows must at least hold
};

// The first field in which the zero-padded plan `p` and the largest submodel's plan `q` lay their blob or state out differently
// ("" = none): everything nam_kq_kernel and nam_kt_mfma_kernel take from a plan but the weights themselves. Equal layouts are
// what lets one launch run both through the bank path (api_bank.cpp compares two bank members the same way).
inline std::string a2_layout_difference(const Plan& p, const Plan& q)
{
  std::string text;
  auto cmp = [&](const char* field, long long x, long long y) {
    if (text.empty() && x != y)
      text = std::string(field) + " (" + std::to_string(x) + " vs " + std::to_string(y) + ")";
  };
  const A1Plan &a = p.a1, &b = q.a1;
  cmp("a1.valid", a.valid, b.valid);
  cmp("in_channels", p.in_channels, q.in_channels);
  cmp("out_channels", p.out_channels, q.out_channels);
  cmp("prewarm_samples", p.prewarm_samples, q.prewarm_samples);
  cmp("state_floats", p.state_floats, q.state_floats);
  cmp("a1_padded_layout", p.a1_padded_layout ? 1 : 0, q.a1_padded_layout ? 1 : 0);
  cmp("blob floats", (long long)p.blob.size(), (long long)q.blob.size());
  cmp("a1.n_arrays", a.n_arrays, b.n_arrays);
  cmp("a1.n_rings", a.n_rings, b.n_rings);
  cmp("a1.head_scale_off", a.head_scale_off, b.head_scale_off);
  for (int r = 0; r < 64 && r < a.n_rings; r++)
    cmp("a1.ring_len_by_id", a.ring_len_by_id[r], b.ring_len_by_id[r]);
  for (int i = 0; i < a.n_arrays && i < kA1MaxArrays; i++)
  {
    const A1Array &x = a.arr[i], &y = b.arr[i];
    cmp("a1.arr.act", x.act, y.act);
    cmp("a1.arr.in_size", x.in_size, y.in_size);
    cmp("a1.arr.channels", x.channels, y.channels);
    cmp("a1.arr.kernel", x.kernel, y.kernel);
    cmp("a1.arr.n_layers", x.n_layers, y.n_layers);
    cmp("a1.arr.head_size", x.head_size, y.head_size);
    cmp("a1.arr.w_base", x.w_base, y.w_base);
    cmp("a1.arr.state_base", x.state_base, y.state_base);
    for (int l = 0; l < x.n_layers && l < kA1MaxLayers; l++)
    {
      cmp("a1.arr.dil", x.dil[l], y.dil[l]);
      cmp("a1.arr.ksize", x.ksize[l], y.ksize[l]);
      cmp("a1.arr.layer_off", x.layer_off[l], y.layer_off[l]);
      cmp("a1.arr.ring_off", x.ring_off[l], y.ring_off[l]);
      cmp("a1.arr.ring_len", x.ring_len[l], y.ring_len[l]);
      cmp("a1.arr.ring_id", x.ring_id[l], y.ring_id[l]);
    }
    cmp("a1.arr.head_k", x.head_k, y.head_k);
    cmp("a1.arr.head_dil", x.head_dil, y.head_dil);
    cmp("a1.arr.head_off", x.head_off, y.head_off);
    cmp("a1.arr.head_ring_off", x.head_ring_off, y.head_ring_off);
    cmp("a1.arr.head_ring_len", x.head_ring_len, y.head_ring_len);
    cmp("a1.arr.head_ring_id", x.head_ring_id, y.head_ring_id);
  }
  cmp("kt_ok", a.kt_ok, b.kt_ok);
  cmp("kp_ok", a.kp_ok, b.kp_ok);
  cmp("kt_chunks", a.kt_chunks, b.kt_chunks);
  cmp("kt_nk", a.kt_nk, b.kt_nk);
  for (int c = 0; c < a.kt_chunks && c < kKtChunkMax; c++)
  {
    const KtDesc &x = a.kt_desc[c], &y = b.kt_desc[c];
    cmp("kt_desc.flags", x.flags, y.flags);
    cmp("kt_desc.ntaps", x.ntaps, y.ntaps);
    cmp("kt_desc.tile_off", x.tile_off, y.tile_off);
    cmp("kt_desc.w1_off", x.w1_off, y.w1_off);
    cmp("kt_desc.consts_off", x.consts_off, y.consts_off);
    cmp("kt_desc.ring_b", x.ring_b, y.ring_b);
    cmp("kt_desc.R", x.R, y.R);
    cmp("kt_desc.ring_id", x.ring_id, y.ring_id);
    for (int i = 0; i < kKtTaps; i++)
      cmp("kt_desc.L", x.L[i], y.L[i]);
  }
  cmp("kt_rech_off", a.kt_rech_off, b.kt_rech_off);
  cmp("kt_lds_src_off", a.kt_lds_src_off, b.kt_lds_src_off);
  cmp("kt_lds_floats", a.kt_lds_floats, b.kt_lds_floats);
  cmp("kq_w_off", a.kq_w_off, b.kq_w_off);
  return text;
}

// The table between `narrow` (the submodel's own plan: its nam_wn_reg_kernel state) and `padded` (its zero-padded plan: the
// largest submodel's rings). !ok when the two do not keep the same rings.
inline A2Transcode build_a2_transcode(const Plan& narrow, const Plan& padded)
{
  A2Transcode t;
  auto refuse = [&](const std::string& why) {
    t.why = why;
    t.rings.clear();
    return t;
  };
  const WrPlan& w = narrow.wr;
  const A1Plan& a = padded.a1;
  if (!w.ok)
    return refuse("the narrow submodel has no nam_wn_reg_kernel plan: " + w.why);
  if (!a.valid || a.n_arrays != 1)
    return refuse("the padded plan is not a single-array A1 plan");
  const A1Array& A = a.arr[0];
  if (A.channels < 1 || A.channels > kA2XcMaxCh)
    return refuse("padded channel count out of range");
  // the narrow side's per-channel rows: the `rows` table, entries {float offset inside the ring area, R, slot | gs << 8, 0}
  if (w.tab_rows < 0 || w.n_rows < 0 || (size_t)w.tab_rows + (size_t)w.n_rows * 4 > w.blob.size())
    return refuse("the rows table lies outside the blob");
  std::vector<int32_t> rows((size_t)w.n_rows * 4);
  if (!rows.empty())
    std::memcpy(rows.data(), w.blob.data() + w.tab_rows, rows.size() * sizeof(int32_t));
  // the ops that keep history, in program order: layer l of the one array, then the head rechannel with taps
  int layer = 0;
  bool head_seen = false;
  for (const WrOp& op : w.ops)
  {
    if (op.type == WR_RUN || op.type == WR_POST_HEAD || op.type == WR_SET_COND)
      return refuse("the narrow program holds an op this table does not describe (a fused run, a post-stack head, a nested condition)");
    if (op.type != WR_LAYER && op.type != WR_ARRAY_END_K)
      continue;
    A2XcRing r;
    std::memset(&r, 0, sizeof(r));
    if (op.type == WR_LAYER)
    {
      if (layer >= A.n_layers || head_seen)
        return refuse("more layers in the narrow program than in the padded plan");
      r.ring_id = A.ring_id[layer];
      r.a2_off = A.ring_off[layer];
      r.R = A.ring_len[layer];
      layer++;
    }
    else
    {
      if (head_seen)
        return refuse("two head rechannels with taps");
      head_seen = true;
      r.ring_id = A.head_ring_id;
      r.a2_off = A.head_ring_off;
      r.R = A.head_ring_len;
    }
    if (r.ring_id < 0) // (kernel size 1 on the padded side: no lookback, nothing the next buffer needs)
    {
      if (op.ring != kBlock)
        return refuse("a ring on the narrow side only");
      continue;
    }
    r.slot = op.slot;
    r.a2_ch = A.channels;
    if (op.ring != r.R)
      return refuse("ring lengths differ: slot " + std::to_string(op.slot) + " keeps " + std::to_string(op.ring) + " frames, ring "
                    + std::to_string(r.ring_id) + " " + std::to_string(r.R));
    if (r.slot < 0 || r.slot >= kWrPosInts || r.ring_id >= kBlock)
      return refuse("write position index out of range");
    for (int e = 0; e < w.n_rows; e++)
    {
      const int32_t* row = &rows[(size_t)e * 4];
      if ((row[2] & 255) != r.slot)
        continue;
      if (r.wr_ch >= r.a2_ch)
        return refuse("the narrow ring has more channels than the padded one");
      if (row[1] != r.R || row[3] != 0)
        return refuse("a rows entry disagrees with its op");
      r.wr_off[r.wr_ch] = kWrPosInts + row[0];
      r.wr_gs[r.wr_ch] = row[2] >> 8;
      r.wr_ch++;
    }
    if (r.wr_ch < 1)
      return refuse("a slot without rows");
    t.rings.push_back(r);
  }
  if (layer != A.n_layers || head_seen != (A.head_ring_id >= 0))
    return refuse("the two plans do not keep the same rings");
  if ((int)t.rings.size() != a.n_rings)
    return refuse("ring counts differ");
  t.wr_state_floats = w.state_floats;
  t.a2_state_floats = padded.state_floats;
  t.ok = true;
  return t;
}

// Walks every float and position word the table names: inside the two states, behind the position tables, no float named twice
// on either side, every ring and slot exactly once. "" = the kernel may run it.
inline std::string a2_transcode_check(const A2Transcode& t)
{
  if (!t.ok)
    return "not built: " + t.why;
  if (t.wr_state_floats < kWrPosInts || t.a2_state_floats < kBlock)
    return "a state smaller than its position table";
  std::vector<char> wr((size_t)t.wr_state_floats, 0), a2((size_t)t.a2_state_floats, 0);
  for (const A2XcRing& r : t.rings)
  {
    if (r.R < kBlock || r.a2_ch < 1 || r.a2_ch > kA2XcMaxCh || r.wr_ch < 1 || r.wr_ch > r.a2_ch)
      return "ring geometry out of range";
    if (r.slot < 0 || r.slot >= kWrPosInts || r.ring_id < 0 || r.ring_id >= kBlock)
      return "position index out of range";
    if (wr[(size_t)r.slot] || a2[(size_t)r.ring_id])
      return "a position word named twice";
    wr[(size_t)r.slot] = a2[(size_t)r.ring_id] = 1;
    if (r.a2_off < kBlock || (long long)r.a2_off + (long long)r.R * r.a2_ch > t.a2_state_floats)
      return "a padded ring outside its state";
    for (long long i = 0; i < (long long)r.R * r.a2_ch; i++)
    {
      if (a2[(size_t)(r.a2_off + i)])
        return "a padded float named twice";
      a2[(size_t)(r.a2_off + i)] = 1;
    }
    for (int c = 0; c < r.wr_ch; c++)
    {
      if (r.wr_gs[c] < 1 || r.wr_gs[c] > 4 || r.wr_off[c] < kWrPosInts)
        return "a narrow row out of range";
      for (long long i = 0; i < r.R; i++)
      {
        const long long f = r.wr_off[c] + i * r.wr_gs[c];
        if (f >= t.wr_state_floats)
          return "a narrow row outside its state";
        if (wr[(size_t)f])
          return "a narrow float named twice";
        wr[(size_t)f] = 1;
      }
    }
  }
  return "";
}

// A container submodel zero-padded onto the layout of the container's largest submodel (plan_a1.cpp). False: not applicable
// (`why` says what stood in the way); true: `out` runs on nam_kq_kernel / nam_kt_mfma_kernel with `full`'s offsets and rings.
bool build_a2_padded_plan(const WaveNetSpec& narrow, const Plan& full, Plan& out, std::string& why);

} // namespace namhip
