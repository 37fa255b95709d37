// launch_policy.h — how many workgroups of nam_wn_reg_kernel a CU holds, up to how many streams a batch keeps the kernel (and a
// session), and how many wavefronts per stream a launch runs with: plain functions of integers. Host only, no HIP header, so
// tests/src/launch_policy_check.cpp asks them at every boundary on the CPU. api_launch.cpp (pick_kernel, launch_wr) and
// api_session.cpp (persist_kind) are the callers.
#pragma once

#include <algorithm>

#include "plan.h"

namespace namhip
{
namespace api
{
constexpr int kCuLdsBytes = 160 * 1024; // a CU's LDS (api_internal.h asserts it is kernels.h: kLdsCu)
constexpr int kPersistTurns = 8; // sessions whose workgroups cannot all be on the chip at once: up to this many turns (they consume the same commands one after the other)

// Workgroups of nam_wn_reg_kernel a CU holds at once: a workgroup is `waves` wavefronts (one per stage of its stream) on the CU's
// four SIMDs at `per_simd` wavefronts each (1; 2: the dense forms), plus `lds_bytes` of LDS, its image (and the queues), counted
// with a margin of 512 bytes.
inline int wr_workgroups_per_cu(int lds_bytes, int waves, int per_simd)
{
  return std::min(4 * per_simd / waves, kCuLdsBytes / (lds_bytes + 512));
}

// A session of nam_wn_reg_kernel exists, and AUTO keeps a plain narrow model on the kernel, up to this many streams: what the chip
// holds as one wavefront per stream, times the turns a session's workgroups may take.
// (pick_kernel used to guard with max(per_cu, 1): a no-op, the planner refuses lds_bytes > kWrMaxLdsBytes, where one still fits.)
inline int wr_stream_bound(int lds_bytes, int cus)
{
  return kPersistTurns * wr_workgroups_per_cu(lds_bytes, 1, 1) * std::max(cus, 1);
}

// Are all `n_wg` workgroups of a launch on the chip at once, when a CU holds `per_cu` of them? What a session's launch needs to
// LINGER (persist_wave.h: wait_command): a workgroup that waits for a slot on a CU consumes nothing while the resident ones wait
// for it, so a launch that runs in turns must leave when its ring is empty. The pipeline kernels' sessions have one workgroup per
// CU (api_internal.h: session_lingers); the one-wavefront-per-workgroup kernels have several, hence this instead of n_wg <= cus.
inline bool launch_all_resident(int n_wg, int per_cu, int cus)
{
  return n_wg >= 1 && per_cu >= 1 && (long)n_wg <= (long)per_cu * std::max(cus, 1);
}
// Workgroups (one wavefront each) of nam_lstm_row_kernel / nam_lstm_wide_kernel a CU holds at once WHATEVER registers the
// instantiation was allocated: one per SIMD (a wavefront may hold a SIMD's whole register file; their LDS, under 12 KB, never
// binds). persist_kind admits more streams than that (the row kernel: eight workgroups per CU); those sessions run in turns.
constexpr int kLstmRowResidentPerCu = 4;
constexpr int kLstmWideResidentPerCu = 4;

struct WrShapeQuery
{
  int total = 0; // workgroups (streams) of the launch
  int lds_bytes = 0; // the largest group's LDS image (WrPlan::lds_bytes)
  int cus = 0; // compute units of the device (0 counts as 1)
  int max_stages = 4; // nam_hip_batch::wr_max_stages
  bool can_split = false, can_split4 = false; // every group's program has the cut for two / the three cuts for four wavefronts
  int dense_forms = 0; // bit 1 / bit 2: the model's code object has a usable dense form of two / four stages (0: none, or no code object of its own)
  bool multi_buffer = false; // the launch holds more than one buffer, so a pipeline has something to overlap (launch_wr)
};
struct WrLaunchShape
{
  int stages = 1; // wavefronts per stream
  bool dense = false; // the two-wavefronts-per-SIMD build of the per-model code object
  int lds_bytes = 0; // of a workgroup: the image + (stages - 1) queues
};

// the launch's relative duration with nst waves per stream: a workgroup is nst waves at `per_simd` waves per SIMD plus its LDS
// image (and the queues), the workgroups beyond what the chip holds run in later turns (persist_kind), and a stream's
// buffer takes 1, 1/1.75, 1/3.1 of the one-wave time (measured: DESIGN 4.5).
// per_simd 2, the DENSE forms of a per-model code object: twice the workgroups per CU; two waves that share a SIMD each issue
// nearly as fast as a lone one — profiles/r05/valu_rate_microbench.txt: 8.6 cycles per instruction of a wave at one AND at two per
// SIMD — minus what they lose to each other's LDS traffic: 0.9
inline double wr_duration(const WrShapeQuery& q, int nst, int per_simd)
{
  const int lds = q.lds_bytes + (nst - 1) * kWrQueueBytes;
  if (lds > kWrMaxLdsBytes)
    return 1e9;
  const int on_chip = std::max(q.cus, 1) * wr_workgroups_per_cu(lds, nst, per_simd);
  const double speed = per_simd == 2 ? 0.9 * (nst == 4 ? 3.1 : 1.75) : nst == 4 ? 3.1 : nst == 2 ? 1.75 : 1.0;
  const int turns = (q.total + on_chip - 1) / on_chip;
  return turns * (1.0 + 0.15 * (turns - 1)) / speed; // a turn's last workgroups leave SIMDs idle; images move in and out
}

// Two or four wavefronts per stream (the program cut up, consecutive buffers in flight: kernel_wn_reg.hip, NST) when the
// launch holds more than one buffer and the chip has the SIMDs for it — config 4's 512 streams become 1,024
// wavefronts, 256 streams too
inline WrLaunchShape wr_launch_shape(const WrShapeQuery& q)
{
  WrLaunchShape out;
  out.lds_bytes = q.lds_bytes;
  if (!q.multi_buffer)
    return out;
  double best = wr_duration(q, 1, 1);
  if (q.can_split && q.max_stages >= 2 && wr_duration(q, 2, 1) < 0.9 * best)
  {
    out.stages = 2;
    best = wr_duration(q, 2, 1);
  }
  if (q.can_split && q.can_split4 && q.max_stages >= 4 && wr_duration(q, 4, 1) < 0.9 * best)
  {
    out.stages = 4;
    best = wr_duration(q, 4, 1);
  }
  // ... or a dense form, ONLY when the best one-per-SIMD form leaves SIMDs without a wavefront (config 5: 768 streams on 1,024
  // SIMDs): where it fills the chip exactly (config 4: 512 streams x 2, 1,024 x 1, 256 x 4) a second wavefront per SIMD only adds
  // hand-overs — measured 3.95 vs 3.87 us (512 streams, four waves per stream dense vs two plain) and 7.59 vs 6.94 (1,024 streams)
  const bool plain_fills = ((long)q.total * out.stages) % (4l * std::max(q.cus, 1)) == 0;
  if (q.can_split && q.max_stages >= 2 && !plain_fills)
  {
    if ((q.dense_forms & 2) && wr_duration(q, 2, 2) < 0.9 * best)
    {
      out.stages = 2;
      out.dense = true;
      best = wr_duration(q, 2, 2);
    }
    if ((q.dense_forms & 4) && q.can_split4 && q.max_stages >= 4 && wr_duration(q, 4, 2) < 0.9 * best)
    {
      out.stages = 4;
      out.dense = true;
    }
  }
  out.lds_bytes += (out.stages - 1) * kWrQueueBytes;
  return out;
}

// ... and whether the launch of that shape holds all its workgroups on the chip at once (wr_duration's `turns` == 1 for the form chosen)
inline bool wr_all_resident(const WrShapeQuery& q, const WrLaunchShape& shape)
{
  return launch_all_resident(q.total, wr_workgroups_per_cu(shape.lds_bytes, shape.stages, shape.dense ? 2 : 1), q.cus);
}

} // namespace api
} // namespace namhip
