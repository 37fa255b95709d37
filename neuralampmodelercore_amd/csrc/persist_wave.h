// persist_wave.h — device side of the persistent block mode for kernels whose workgroup is ONE wavefront
// (nam_wn_reg_kernel, nam_lstm_row_kernel). The protocol is the one nam_a1_p2_kernel speaks (kernel_a1_p2.hip, PERSIST;
// host side: api_session.cpp; api_internal.h: PersistSession): the launch consumes COMMANDS — one per buffer of 1 .. 64 frames,
// `(seq << 32) | frame offset` for a whole one, the frame count on top of a shorter tag for a partial one (session_command.h) — in
// a ring the host (or the caller's stream) stores into, for as long as the next one is already there
// when a buffer is finished, and leaves as soon as the ring is empty (it never waits unboundedly: a device-wide
// synchronize must not depend on a command arriving). A wavefront of its own needs no agreement step: every lane
// reads the same ring word.
//
// A session whose results go to host memory for ticketed buffers or back-to-back blocking calls PUBLISHES every command
// (PersistArgs::cmd_done != nullptr): the workgroup that has stored command c's output counts itself in, the last one through
// stores c + 1 to the host's completion word of the command (complete()), so a wait returns while the launch runs on. Such a
// launch may also LINGER (PersistArgs::linger > 0): a workgroup that finds the ring empty waits for the next command for a
// bounded time under the rules of the pipeline kernels' sessions (wait_command() mirrors il_common.h: session_wait_command,
// leaving() mirrors session_leaving) instead of leaving at once, so the next buffer finds the launch still there. A launch
// that does not publish (device windows, hosts that flush) takes none of these paths: one wavefront-uniform test per command.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "session_command.h"

namespace namhip
{

struct PersistWave
{
  unsigned seq = 0; // commands consumed so far
  unsigned long long spec = 0; // the early look at the next command

  static __device__ __forceinline__ unsigned long long ring_load(const PersistArgs& p, unsigned s)
  {
    const unsigned long long v = __hip_atomic_load(p.ring + (s & (unsigned)p.ring_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // wavefront-uniform (every lane loaded the same word): keep it in scalar registers
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
  }
  // is `v` command number `tag`? (wavefront-uniform scalar arithmetic, once per command)
  static __device__ __forceinline__ bool is_command(unsigned long long v, unsigned tag) { return session::tag_of_hi((unsigned)(v >> 32)) == tag; }
  // does the early look already show the command next() will hand out (number seq + 2 while seq + 1 is being processed)? Its
  // offset and frame count, for a prefetch of its input
  __device__ __forceinline__ bool peek(unsigned& frame_off, int& n_frames) const
  {
    frame_off = (unsigned)spec;
    n_frames = session::frames_of_hi((unsigned)(spec >> 32));
    return is_command(spec, seq + 2u);
  }
  // the first command of this launch (its frame offset and its frame count, 1 .. 64); false = nothing to do (its predecessor
  // consumed the command it was started for)
  __device__ __forceinline__ bool begin(const PersistArgs& p, int wg, unsigned& frame_off, int& n_frames)
  {
    if (p.seq0 >= 0) // every workgroup stands at the same count: it and the first command came with the launch
    {
      seq = (unsigned)p.seq0;
      frame_off = (unsigned)p.cmd0;
      n_frames = session::frames_of_hi((unsigned)(p.cmd0 >> 32));
      return true;
    }
    seq = (unsigned)__builtin_amdgcn_readfirstlane((int)p.cons[wg]);
    unsigned long long v = ring_load(p, seq);
    if (p.linger > 0)
    {
      // a launch that lingers (the host set grace >= linger): a workgroup that finds itself up to date — another one's backlog
      // was the reason for the launch — stays for the commands to come, under wait_command's rules
      v = wait_command(p, seq + 1, v, (long long)p.grace);
      if (!is_command(v, seq + 1))
        leaving(p);
    }
    else if (p.grace > 0 && !is_command(v, seq + 1))
    {
      // started right behind a stream-ordered command store on another hardware queue: look for a bounded time
      const long long t_end = (long long)wall_clock64() + p.grace;
      do
      {
        __builtin_amdgcn_s_sleep(8);
        v = ring_load(p, seq);
      } while (!is_command(v, seq + 1) && (long long)wall_clock64() < t_end);
    }
    frame_off = (unsigned)v;
    n_frames = session::frames_of_hi((unsigned)(v >> 32));
    return is_command(v, seq + 1);
  }
  // while a buffer is being processed: request the next command (consumed by next())
  __device__ __forceinline__ void look_ahead(const PersistArgs& p) { spec = ring_load(p, seq + 1); }
  // A lingering launch waits for command `tag` (ring slot of sequence number tag - 1; `v`: what the slot held at the last look)
  // for `window` ticks of the 100 MHz clock. The twin of il_common.h: session_wait_command for one-wavefront workgroups, rule for
  // rule: the host's "leave" word behind the ring (= the session's command count: nothing follows) ends the wait at once; when
  // the window has passed the workgroup stays only while another workgroup is BEHIND it (cmd_count[mask + 1]: the highest command
  // every workgroup is through) and no workgroup of this launch has left (cmd_count[mask + 2]); 20 ms at the very most, so a
  // device-wide synchronize never depends on a command arriving. Every lane reads the same words: the branches are uniform.
  static __device__ __forceinline__ unsigned long long wait_command(const PersistArgs& p, const unsigned tag, unsigned long long v, const long long window)
  {
    if (is_command(v, tag) || window <= 0)
      return v;
    const long long t0 = (long long)wall_clock64(), t_end = t0 + window, t_cap = t0 + 2000000ll;
    for (;;)
    {
      __builtin_amdgcn_s_sleep(16);
      v = ring_load(p, tag - 1u);
      if (is_command(v, tag))
        break;
      const long long now = (long long)wall_clock64();
      const unsigned gone = (unsigned)__builtin_amdgcn_readfirstlane(
        (int)(unsigned)__hip_atomic_load(p.ring + p.ring_mask + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
      if (gone == tag - 1u)
        break;
      if (now >= t_end)
      {
        const unsigned all_done = (unsigned)__builtin_amdgcn_readfirstlane(
          (int)__hip_atomic_load(p.cmd_count + p.ring_mask + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const unsigned left = (unsigned)__builtin_amdgcn_readfirstlane(
          (int)__hip_atomic_load(p.cmd_count + p.ring_mask + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (now >= t_cap || (int)(all_done - (tag - 1u)) >= 0 || left != 0u)
          break;
      }
    }
    return v;
  }
  // ... and a workgroup of a lingering launch that leaves says so (one lane; the twin of il_common.h: session_leaving)
  static __device__ __forceinline__ void leaving(const PersistArgs& p)
  {
    if (p.linger > 0 && (threadIdx.x & 63u) == 0u)
      __hip_atomic_fetch_add(p.cmd_count + p.ring_mask + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // a buffer is finished: the next command, or false when the ring is empty (the caller then leaves)
  __device__ __forceinline__ bool next(const PersistArgs& p, int wg, unsigned& frame_off, int& n_frames)
  {
    seq++;
    if ((seq & 15u) == 0u && threadIdx.x == 0) // progress for the host's ring bookkeeping (no fence: not a completion signal)
      __hip_atomic_store(p.prog + wg, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    unsigned long long v = spec;
    if (!is_command(v, seq + 1))
    {
      v = ring_load(p, seq); // the early look missed: once more, now
      if (p.linger > 0) // (wavefront-uniform) ... and, a launch that lingers, for a while
      {
        v = wait_command(p, seq + 1, v, (long long)p.linger);
        if (!is_command(v, seq + 1))
          leaving(p);
      }
    }
    frame_off = (unsigned)v;
    n_frames = session::frames_of_hi((unsigned)(v >> 32));
    return is_command(v, seq + 1);
  }
  // Command number `c` (counted from 0: the one taken with seq == c) is finished and this workgroup's output of it is stored:
  // publish it when the launch does that (wavefront-uniform test; called by the wavefront that stored the output). Results
  // visible to the host first (system-scope release fence), then one lane counts the workgroup in (agent scope); the workgroup
  // that finds everybody else there — with ONE workgroup that is the first through — zeroes the counter for the slot's next use,
  // stores c + 1 to the host's completion word and raises "the highest command everybody is through" (wait_command's second rule).
  static __device__ __forceinline__ void complete(const PersistArgs& p, unsigned c)
  {
    if (p.cmd_done == nullptr)
      return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    const unsigned slot = c & (unsigned)p.ring_mask;
    unsigned before = 0u;
    if ((threadIdx.x & 63u) == 0u)
      before = __hip_atomic_fetch_add(p.cmd_count + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)__builtin_amdgcn_readfirstlane((int)before) == gridDim.x - 1u)
    {
      // (the others' fences stand in front of their counts: this one orders their results, seen through the counter, in front of the word)
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "");
      if ((threadIdx.x & 63u) == 0u)
      {
        __hip_atomic_store(p.cmd_count + slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.cmd_done + slot, c + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_fetch_max(p.cmd_count + p.ring_mask + 1, c + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  // results visible, then the consumed-command count: device copy for this workgroup's next launch, host copy (with
  // the "left" bit) for the host
  __device__ __forceinline__ void leave(const PersistArgs& p, int wg)
  {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (threadIdx.x == 0)
    {
      p.cons[wg] = seq;
      __hip_atomic_store(p.done + wg, seq | 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
};

// an input sample of a persistent session: past the caches (the caller may rewrite the same buffer between two commands
// and no kernel boundary invalidates what this CU read a buffer ago)
__device__ __forceinline__ float persist_in(const float* p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

} // namespace namhip
