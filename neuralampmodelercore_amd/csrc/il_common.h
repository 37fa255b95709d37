// il_common.h — helpers shared by the interleaved-frame kernels (kernel_a1_p2.hip and the pipelines built on its lane layout and
// session protocol: kernel_a1_p4.hip, kernel_a1_q.hip, kernel_kq.hip); kernel_kt_mfma.hip includes it for weights_of,
// kernel_lstm.hip for for_each_index. The job table of the A1 kernels is plan.h's namespace p2, compile-time constants; the plan
// compiler admits a model only if its geometry is what those say (plan_a1.cpp: build_a1_il), and topologies outside them run
// nam_a1_mfma_kernel. What it holds:
//   * the lane-layout pieces: Slot / Ops, row_shr / dpp_taps, for_each_index, kOob;
//   * weights_of<BANK>: what a workgroup reads its weights from (one model or a bank member);
//   * the pipelines' ring addressing, once: i4 / sb_load4 / sb_store4 (the struct-buffer intrinsics), ring_desc, wrap_row /
//     wrap_s, stage_write_positions, and wait_lds_word (p4's and kq's LDS word wait; q's scalar-unit form stays in q);
//   * session_wait_command / session_leaving: how a session launch waits for its next command.
// Each kernel keeps its own stream prologue (stream, state, input / output rows and their descriptors): moved into a shared
// helper it compiles to other device code in p4 and kq (profiles/il_prologue/README.md).
#pragma once
#include "device_common.h"

#include <utility>

namespace namhip
{
namespace il
{
using mf::f2;
using mf::f4;
using u4 = __attribute__((ext_vector_type(4))) unsigned;
struct Slot
{
  f4 a, b; // raw ring rows (16 bytes of the lane's channel quad) of the job's two requests
  float inp; // input sample of the lane's frame in the block the job belongs to (every job carries it: a load inside
             // an `if (block boundary)` would turn every counted vmcnt wait behind it into vmcnt(0))
};
struct Ops // one job's register-resident operands
{
  f4 t[4]; // A tiles: conv tap 0, 1, 2 | layer1x1
  f4 xt; // extra tile (rechannel / head rechannel)
  f4 bv, mv, b1v, ev; // conv bias | input mixin | 1x1 bias | extra
  int ready; // loader progress word as read just before the operands
};
constexpr unsigned kOob = 0x7ffffff0u; // beyond num_records: loads return 0, stores are dropped, no memory traffic

template <int N>
__device__ __forceinline__ float row_shr(float old, float src)
{
  // lane i of a 16-lane row receives src of lane i - N; lanes i < N keep `old`
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src),
                                                               0x110 + N, 0xf, 0xf, false));
}
// taps of a layer with dilation 4 * N1 from the lane's own registers: tap 1 = frame t - d (N1 lanes down the row),
// tap 0 = frame t - 2d (2 N1 lanes down; a whole row = the previous block's same lane). `pa` / `pb`: the previous
// block's values for the lanes that fall off the row. NV values per lane (4: full layout, 2: half layout).
template <int NV, int N1>
__device__ __forceinline__ void dpp_taps(const f4& x, const f4& pa, const f4& pb, f4& bt0, f4& bt1)
{
#pragma unroll
  for (int e = 0; e < NV; e++)
  {
    bt1[e] = row_shr<N1>(pb[e], x[e]);
    if constexpr (2 * N1 < 16)
      bt0[e] = row_shr<2 * N1>(pa[e], x[e]);
    else
      bt0[e] = pa[e];
  }
}
// f(std::integral_constant<int, 0>{}), f(<1>), ... f(<N-1>) in order: a compile-time unrolled job sequence
template <class F, int... I>
__device__ __forceinline__ void for_each_index(F&& f, std::integer_sequence<int, I...>)
{
  (f(std::integral_constant<int, I>{}), ...);
}

// What a workgroup reads its weights and per-model scalars from. BANK (a model bank: A1Args::bank_member): the stream's member is
// resolved once, wave-uniformly (scalar loads), right after the stream itself; nothing behind the prologue depends on it.
// !BANK: the launch's one model, straight from the kernel arguments — the code of those instantiations does not change.
struct Weights
{
  const float* blob;
  float head_scale, act_p0;
};
template <bool BANK>
__device__ __forceinline__ Weights weights_of(const float* __restrict__ blob, const A1Args& a, int stream)
{
  if constexpr (BANK)
  {
    const int m = uni(a.bank_member[stream]);
    const float* sc = a.bank_scal + 2 * m;
    return Weights{blob + (size_t)m * (size_t)a.bank_stride, __builtin_bit_cast(float, uni(__builtin_bit_cast(int, sc[0]))),
                   __builtin_bit_cast(float, uni(__builtin_bit_cast(int, sc[1])))};
  }
  else
    return Weights{blob, a.head_scale, a.act_p0};
}

// MUBUF with index AND offset registers (address = base + soffset + index * stride + offset): the ring row index goes
// in as it is — no multiply / shift / add per address — and an index beyond num_records makes the access a no-op. clang
// has builtins for the raw form only; the LLVM intrinsics are declared by name (the compiler's wait-count bookkeeping
// covers them like any other vector-memory instruction).
using i4 = __attribute__((ext_vector_type(4))) int;
__device__ f4 sb_load4(i4 rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.load.v4f32");
__device__ void sb_store4(f4 v, i4 rsrc, int vindex, int voffset, int soffset, int aux) __asm("llvm.amdgcn.struct.buffer.store.v4f32");

// A descriptor of the stream's rings with the row pitch as the stride (64 bytes: 16-channel rows, 32 bytes: 8-channel rows
// ...): an access names its row by INDEX and its ring by the scalar offset. `rows` = num_records, far above every real row
// index: an index no descriptor holds (the kernels' kNoRow) drops the access / returns 0 without a compare.
__device__ __forceinline__ i4 ring_desc(const float* st, int row_b, int rows)
{
  const unsigned long long st_addr = (unsigned long long)st;
  return i4{uni((int)(unsigned)st_addr), uni((int)((unsigned)(st_addr >> 32) & 0xffffu) | (row_b << 16)), rows, 0x00020000};
}
// row (sb + off) mod R for a wave-uniform sb in [0, R) and a lane offset below 64 <= R (kNoRow on either side stays beyond
// num_records)
__device__ __forceinline__ unsigned wrap_row(int sb, unsigned off, unsigned R)
{
  const unsigned v = (unsigned)sb + off;
  return min(v, v - R);
}
__device__ __forceinline__ int wrap_s(int v, int R) // wave-uniform, v in (-R, R)
{
  v += v < 0 ? R : 0;
  return v;
}
// The write positions of stage S's rings as SCALARS, advanced on the scalar unit from here on: wp[u] = ring of job
// FIRST_JOB(S) + u, from wposv (lane r = write position of ring r = job r). FIRST_JOB(s): first job of stage s, stage NST = end.
// (S and wposv by reference and plain `inline`: by value the pipelines' register allocation moves.)
template <int NST, int (*FIRST_JOB)(int), int MAXJ>
__device__ inline void stage_write_positions(const int& S, const int& wposv, int (&wp)[MAXJ])
{
  for_each_index(
    [&](auto s_tag) {
      constexpr int SS = decltype(s_tag)::value;
      if (S == SS)
      {
        constexpr int J0 = FIRST_JOB(SS), NJS = FIRST_JOB(SS + 1) - J0;
#pragma unroll
        for (int u = 0; u < MAXJ; u++)
          wp[u] = u < NJS ? __builtin_amdgcn_readlane(wposv, J0 + (u < NJS ? u : 0)) : 0;
      }
    },
    std::make_integer_sequence<int, NST>{});
}
// Until the LDS word at byte_addr has reached `want`. The pipelines' synchronisation words have ONE writer each (plain
// stores, no atomics); the waiting side polls from inline asm — a wait loop in C++ is a LOOP to the compiler: it splits the
// live ranges of the request slots around it, shuffles them with copies at the joins and drains every ring request in flight
// (vmcnt(0)) to do so; an asm statement is straight-line code. One wave's LDS operations execute in program order: "data,
// then flag" needs nothing in between.
__device__ __forceinline__ void wait_lds_word(unsigned byte_addr, int want)
{
  int tmp;
  asm volatile("1:\n\tds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)\n\tv_sub_u32 %0, %0, %2\n\tv_cmp_gt_i32 vcc, 0, %0\n\t"
               "s_cbranch_vccz 2f\n\ts_sleep 1\n\ts_branch 1b\n2:"
               : "=&v"(tmp)
               : "v"(byte_addr), "v"(want)
               : "vcc");
}
} // namespace il

// A session launch waits for command `tag` (ring slot of sequence number tag - 1; `v` = what the slot held at the last look) for
// `window` ticks of the 100 MHz clock. A launch that LINGERS (ticketed host buffers: A1Args::p_linger > 100; nam_a1_q_kernel,
// nam_kq_kernel) has two more rules:
//  * the host's "leave" word behind the ring (= the session's command count: nothing follows) ends the wait at once;
//  * when the window has passed, the workgroup still stays while another workgroup is BEHIND it — p_cmd_count[mask + 1] holds
//    the highest command every workgroup is through (atomic max by the last one through each). The host hands the next buffer
//    in when the slowest workgroup has finished an old one; a workgroup that left meanwhile would miss it, the rest would have
//    to run dry, linger and leave before the next launch could pick it up again — and then the two halves take turns being the
//    one that left (measured: 1,024-frame buffers at 27 k xRT instead of 57 k, a relaunch per 16 buffers). Not once a workgroup
//    of this launch HAS left (p_cmd_count[mask + 2], cleared by the host in front of every launch: session_leaving): the one
//    behind may be the one that is gone. Capped at 20 ms.
template <int SLEEP, class RingLoad>
__device__ __forceinline__ unsigned long long session_wait_command(const A1Args& a, RingLoad ring_load, const unsigned tag, unsigned long long v,
                                                                  const long long window)
{
  if ((unsigned)(v >> 32) == tag || window <= 0)
    return v;
  const bool lingers = a.p_linger > 100;
  const long long t0 = (long long)wall_clock64(), t_end = t0 + window, t_cap = t0 + (lingers ? 2000000ll : window);
  int why = 0; // (developer statistics: why the wait ended without a command — NAM_HIP_SESSION_STATS, a.dbg = a host-mapped array)
  for (;;)
  {
    __builtin_amdgcn_s_sleep(SLEEP);
    v = ring_load(tag - 1u);
    if ((unsigned)(v >> 32) == tag)
      break;
    const long long now = (long long)wall_clock64();
    if (!lingers)
    {
      if (now >= t_end)
        break;
      continue;
    }
    if ((unsigned)__hip_atomic_load(a.p_ring + a.p_ring_mask + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == tag - 1u)
    {
      why = 1;
      break;
    }
    if (now >= t_end)
    {
      const unsigned all_done = __hip_atomic_load(a.p_cmd_count + a.p_ring_mask + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      why = now >= t_cap ? 2 : (int)(all_done - (tag - 1u)) >= 0 ? 3 : __hip_atomic_load(a.p_cmd_count + a.p_ring_mask + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 4 : 0;
      if (why)
      {
        if (a.dbg && a.p_ring)
          a.dbg[blockIdx.x] = ((long long)why << 56) | ((long long)(SLEEP == 8 ? 1 : 0) << 48) | ((long long)(all_done & 0xffffffu) << 24) | (long long)((tag - 1u) & 0xffffffu);
        break;
      }
    }
  }
  (void)why;
  return v;
}
// ... and a workgroup of a lingering launch that leaves says so (one lane)
__device__ __forceinline__ void session_leaving(const A1Args& a)
{
  if (a.p_linger > 100)
    __hip_atomic_fetch_add(a.p_cmd_count + a.p_ring_mask + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
} // namespace namhip
