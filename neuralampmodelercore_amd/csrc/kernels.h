// kernels.h — kernel argument blocks and host-side launch wrappers (kernel_*.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <type_traits>

#include "a2_transcode.h"
#include "linear_worklist.h"
#include "plan.h"

namespace namhip
{

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the CURRENT DEVICE's copy of a function: a process that runs
// batches on several GPUs must raise it once per (function, device). One of these per kernel instantiation; devices
// beyond 63 set the attribute on every launch.
struct DynamicLdsLimit
{
  unsigned long long raised = 0; // bit d: done on device d (launches of one batch come from one host thread at a time;
                                 // a lost update between threads only repeats the call)
  hipError_t ensure(const void* fn, int bytes)
  {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
      return e;
    const bool tracked = dev >= 0 && dev < 64;
    if (tracked && ((__atomic_load_n(&raised, __ATOMIC_RELAXED) >> dev) & 1ull))
      return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && tracked)
      __atomic_fetch_or(&raised, 1ull << dev, __ATOMIC_RELAXED);
    return e;
  }
};

// Where a session-capable kernel is launched. A session's resident launch carries its own completion signal: persist_launch
// (api_session.cpp) hands the session's event down as `retired`, and hipExtLaunchKernelGGL puts the event's signal on the
// dispatch packet itself, so the host's wait for "the launch has retired" (nam_hip_batch_flush, synchronize, the end of a
// session) is a wait on that signal: ~1.4 us behind the last workgroup instead of the ~11 us a stream / device synchronize
// takes to push a marker packet through the queue behind a plain launch (tools/src/sync_tail.hip, profiles/r05/sync_tail.txt).
// nullptr: a plain launch. The other kernels' wrappers take a hipStream_t (it converts WITHOUT an event): nobody can hand them one.
struct LaunchStream
{
  hipStream_t stream;
  hipEvent_t retired;
  LaunchStream(hipStream_t s, hipEvent_t r = nullptr) : stream(s), retired(r) {}
};

// One kernel instantiation on the current device, its dynamic-LDS limit raised to `lds_ceiling`: the limit object lives here, one
// per `Kernel` (= per instantiation, as DynamicLdsLimit asks). Also what a first launch would otherwise pay for (~1.6 ms: the
// code object).
constexpr int kLdsDefault = 64 * 1024; // what a launch may ask for without the attribute
constexpr int kLdsCu = 160 * 1024; // a CU's LDS
template <auto Kernel>
inline hipError_t instance_ready(int lds_ceiling)
{
  static DynamicLdsLimit lds_limit;
  return lds_limit.ensure(reinterpret_cast<const void*>(Kernel), lds_ceiling);
}
// ... and launched: with the session's completion event on the dispatch when `s` carries one, else plainly — as every launch
// on a bare hipStream_t is (LaunchStream). DynamicLdsLimit records "raised", not a size: a kernel whose LDS request differs
// from launch to launch names the most it may ask for as kLdsCeiling
// (0: every launch of the instantiation asks for the same lds_bytes). kLdsDefault as the ceiling is a refusal bound only: those
// kernels never need the attribute raised, and one call per device that sets what is the default anyway costs nothing.
template <auto Kernel, int kLdsCeiling = 0, typename... Args>
inline hipError_t launch_instance(dim3 grid, dim3 block, int lds_bytes, LaunchStream s, Args... args)
{
  if (kLdsCeiling && lds_bytes > kLdsCeiling)
    return hipErrorInvalidValue;
  const hipError_t e = instance_ready<Kernel>(kLdsCeiling ? kLdsCeiling : lds_bytes);
  if (e != hipSuccess)
    return e;
  if (s.retired)
    hipExtLaunchKernelGGL(Kernel, grid, block, lds_bytes, s.stream, nullptr, s.retired, 0, args...);
  else
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s.stream, args...);
  return hipGetLastError();
}

// Persistent session of a one-wavefront-per-workgroup kernel (persist_wave.h); ring == nullptr: an ordinary launch
struct PersistArgs
{
  unsigned long long* ring = nullptr; // commands: (seq << 32) | frame offset
  int ring_mask = 0; // ring size - 1
  unsigned* cons = nullptr; // device memory: commands consumed per workgroup (where its next launch resumes)
  unsigned* prog = nullptr; // host-mapped: progress (every 16 commands)
  unsigned* done = nullptr; // host-mapped: consumed count | "left" bit, written when the workgroup leaves
  long long seq0 = -1; // >= 0: every workgroup has consumed exactly this many commands (cons is not read) ...
  unsigned long long cmd0 = 0; // ... and this is the next command (the ring is not read for it)
  int grace = 0; // ticks (100 MHz) a fresh launch looks for its first command before it leaves again
  // Per-command completion, as A1Args::p_cmd_count / p_cmd_done / p_linger (persist_wave.h: complete, wait_command).
  // cmd_done == nullptr: the launch does not publish — none of the three is read, and the kernels run what they always ran.
  int linger = 0; // ticks (100 MHz) a workgroup that finds the ring empty looks for the next command before it leaves; 0 = it leaves at once
  unsigned* cmd_count = nullptr; // device memory: [c & ring_mask] workgroups through command c (zero between uses); [ring_mask + 1] the highest
                                 // command every workgroup is through; [ring_mask + 2] workgroups of this launch that have left (the host clears it per launch)
  unsigned* cmd_done = nullptr; // host-mapped: [c & ring_mask] = c + 1, stored by the last workgroup through command c behind everybody's results
  // (the host's "leave" word of a lingering launch is ring[ring_mask + 1]; the launch's workgroup count is its grid)
};

// I/O convention for every kernel: planar float32 in HBM,
//   in [stream][in_ch ][io_stride]   out [stream][out_ch][io_stride]
// of which frames [0, n_frames) are processed by this launch (the caller may point `in`/`out` into
// the middle of a longer resident buffer; io_stride is the row pitch in floats).
// `in == nullptr` means silence (prewarm); `out == nullptr` discards the output.
struct GenericArgs
{
  const NamOp* ops;
  const float* blob;
  float* state;
  long state_stride; // floats per stream
  const int* stream_map; // optional: blockIdx -> stream index (mixed-width batches); nullptr = identity
  const float* in;
  float* out;
  long io_stride;
  int n_frames;
  int in_ch, out_ch;
  // weights in LDS: the first blob_floats floats of the blob are copied behind the activation rows (float offset
  // w_lds_off) once per launch and conv weights are read from there (broadcast ds_reads: ~64 cycles, pipelined in
  // order) instead of through scalar loads (~200+ cycles each, not pipelinable across uses); 0 = keep scalar loads
  int w_lds_off, blob_floats;
};

struct A1Args
{
  const A1Plan* plan; // device copy
  const float* blob;
  float* state;
  long state_stride;
  const int* stream_map;
  const float* in;
  float* out;
  long io_stride;
  int n_frames;
  float act_p0; // LeakyReLU slope when the arrays use it
  // MFMA kernel: host-known scalars passed by value so the kernel prologue has no dependent loads
  int n_rings, n_mjobs = 0;
  int tiles_off = 0, consts_off = 0; // blob offsets (floats) of the tile areas / consts table
  float head_scale;
  // wave-specialised kernel
  int r1_off = 0; // blob offset of the first array's rechannel column (16 floats)
  int xt_off = 0, n_xt = 0; // blob offset / count of the extra tiles
  int lds_tiles_b = 0, lds_xt_b = 0, lds_cond_b = 0, lds_bytes = 0; // dynamic LDS layout (bytes)
  int prefetch = 0; // the plan's ws_prefetch (mover prefetch depth the descriptors were built for)
  int act = 0; // the arrays' activation type when it is uniform (nam_a1_p2_kernel's run-time-dispatch instantiation)
  // persistent session of nam_a1_p2_kernel (nullptr = ordinary launch): command ring in device memory, ring size - 1,
  // commands consumed before this launch, per-workgroup progress / completion words in host-mapped memory
  unsigned long long* p_ring = nullptr;
  int p_ring_mask = 0;
  unsigned* p_cons = nullptr; // device memory: commands consumed per workgroup (where its next launch resumes)
  unsigned* p_prog = nullptr; // host-mapped: progress, stored every 16 commands — the host's ring bookkeeping (back-pressure), NEVER a completion signal
                    // (per-buffer completion: p_cmd_done below; the launch's own: p_done = count | exited bit)
  unsigned* p_done = nullptr;
  long long p_seq0 = -1; // >= 0: every workgroup has consumed exactly this many commands (p_cons is not read) ...
  unsigned long long p_cmd0 = 0; // ... and this is the next command (the ring is not read for it)
  int p_grace = 0; // ticks (100 MHz) a fresh launch looks for its first doorbell before it leaves again
  int p_out_host = 0; // the session's output window is HOST memory (nam_a1_p4_kernel: kOutHost — plain result stores, ring
                  // appends written through, one system-scope release fence before the completion word). 2 (nam_a1_q_kernel,
                  // nam_kq_kernel): ticketed host buffers — results written through and p_cmd_done stored after EVERY command,
                  // behind the results: the host takes a buffer's output while the launch runs on (nam_hip_batch_wait_f32)
  int p_linger = 0; // ticks (100 MHz) the launch looks for the NEXT command when it finds the ring empty, before it leaves (nam_a1_q_kernel,
                // nam_kq_kernel; 0 = 1 us, the other kernels' constant): a ticket session's host hands a buffer in every 5 - 15 us
  // ticketed host buffers (p_out_host == 2): p_cmd_count[c & p_ring_mask] (device memory) counts the workgroups that have finished
  // command c and made its results visible; the last one zeroes it and stores c + 1 to p_cmd_done[c & p_ring_mask] (host-mapped):
  // ONE word for the host to poll per buffer, one PCIe write per command
  unsigned* p_cmd_count = nullptr;
  unsigned* p_cmd_done = nullptr;
  long long* dbg; // optional: per-job phase timestamps of workgroup 0 (profiling builds / tools only), else nullptr
  // model bank (nam_hip_batch_create_bank; nam_a1_q_kernel, nam_a1_p4_kernel, nam_a1_p2_kernel — their BANK instantiations;
  // nullptr = one model, the fields above): stream s runs member m = bank_member[s] of `blob` = [members][bank_stride] floats
  // (a multiple of four: the kernels read 16-byte records), with head_scale = bank_scal[2 m] and act_p0 = bank_scal[2 m + 1].
  // The offsets above are the same for every member (api_bank.cpp compares the plans). Read once, in the prologue.
  const int* bank_member;
  const float* bank_scal;
  long bank_stride;
};
static_assert(sizeof(A1Args) == 248, "A1Args is a kernel argument (256 bytes of kernarg with the blob pointer in front): its layout is part of the compiled kernels");

// Which instantiation of a session-capable pipeline kernel (nam_a1_p4_kernel, nam_a1_q_kernel, nam_kq_kernel) a launch takes
// besides its model's: f(WT, PERSIST) with the two as std::bool_constant.
// A session's launch (PERSIST) appends to its rings write-back — written through, the rows a block appends would be read back
// from memory instead of the L2 one block later: 27 us per block instead of 10.5, measured — unless its results go to host
// memory (A1Args::p_out_host); an ordinary launch writes ring appends through when it is short (device_common.h: ring_store).
template <typename F>
inline hipError_t with_session_form(bool session, bool out_host, int n_frames, F&& f)
{
  constexpr std::true_type yes;
  constexpr std::false_type no;
  if (session)
    return out_host ? f(yes, yes) : f(no, yes);
  return n_frames <= 2 * kBlock ? f(yes, no) : f(no, no);
}

struct LSTMArgs
{
  const float* blob;
  float* state;
  long state_stride;
  const int* stream_map; // optional: launch position -> stream index; nullptr = identity
  const float* in;
  float* out;
  long io_stride;
  int n_frames;
  int n_streams;
  int n_layers, input_size, hidden, in_ch, out_ch, fast;
  int head_w, head_b;
  int layer_w[16];
  int layer_b[16];
  // nam_lstm_mfma_kernel (plan.h: LSTMPlan::mf_*)
  int mf_off, mf_floats, mf_nt, mf_head_tiles, mf_head_bias, mf_lds_bytes;
  int mf_layer_tiles[16];
  int mf_layer_bias[16];
  PersistArgs ps; // nam_lstm_row_kernel / nam_lstm_wide_kernel
  float* scratch = nullptr; // nam_lstm_kernel<true>: global-memory h / c / gate columns (lstm_scratch_floats)
  // model bank (nam_hip_batch_create_bank; the BANK instantiations of nam_lstm_row_kernel / nam_lstm_wide_kernel; nullptr = one
  // model): stream s runs member m = bank_member[s] of `blob` = [members][bank_stride] floats (whole plan blobs, a multiple of
  // four). The offsets above are the same for every member (api_bank.cpp compares the plans). Read in the prologue only. Behind
  // every other field: the one-model instantiations find theirs where they were.
  const int* bank_member = nullptr;
  long bank_stride = 0;
};
// the model's part of an LSTM launch's arguments; the caller adds the streams and the audio
inline LSTMArgs lstm_args(const LSTMPlan& L)
{
  LSTMArgs a;
  a.n_layers = L.n_layers;
  a.input_size = L.input_size;
  a.hidden = L.hidden;
  a.in_ch = L.in_ch;
  a.out_ch = L.out_ch;
  a.fast = L.fast;
  a.head_w = L.head_w;
  a.head_b = L.head_b;
  a.mf_off = L.mf_off;
  a.mf_floats = L.mf_floats;
  a.mf_nt = L.mf_nt;
  a.mf_head_tiles = L.mf_head_tiles;
  a.mf_head_bias = L.mf_head_bias;
  a.mf_lds_bytes = L.mf_lds_bytes;
  for (int i = 0; i < 16; i++)
  {
    a.layer_w[i] = L.layer_w[i];
    a.layer_b[i] = L.layer_b[i];
    a.mf_layer_tiles[i] = L.mf_layer_tiles[i];
    a.mf_layer_bias[i] = L.mf_layer_bias[i];
  }
  return a;
}
// Which cells the small-LSTM kernels take, and which the matrix-core kernel keeps in registers. Written over LSTMPlan's
// fields; LSTMArgs carries a copy of them (lstm_args), so the launch_lstm_* guards ask the same functions (`L`: either).
template <typename L>
inline bool lstm_small_io(const L& l) // one or two layers over one or two input channels, at most 16 outputs
{
  return l.n_layers >= 1 && l.n_layers <= 2 && l.input_size >= 1 && l.input_size <= 2 && l.in_ch == l.input_size && l.out_ch >= 1
         && l.out_ch <= 16;
}
template <typename L>
inline bool lstm_row_eligible(const L& l) // nam_lstm_row_kernel
{
  return l.hidden >= 1 && l.hidden <= 4 && lstm_small_io(l);
}
template <typename L>
inline bool lstm_wide_eligible(const L& l) // nam_lstm_wide_kernel
{
  return l.hidden >= 5 && l.hidden <= 32 && lstm_small_io(l);
}
template <typename L>
inline bool lstm_mfma_in_registers(const L& l) // nam_lstm_mfma_reg_kernel: everything in registers (only the I/O tiles in LDS)
{
  return l.input_size <= 4 && l.n_layers <= 2 && l.mf_nt <= 6;
}

// Linear (plan.h: LinearPlan; kernel_linear.hip). One PIECE of a launch: n_frames <= the batch's piece length.
struct LinearArgs
{
  const float* blob; // the padded taps (LinearPlan)
  float* hist; // [hist_frames][cols_pad]: the batch's input history, a ring; row `pos` receives frame 0 of this piece
  float* part; // [n_splits][part_frames][cols_pad]: the splits' partial sums of this piece
  const float* in; // planar [stream][in_ch][io_stride], nullptr = silence
  float* out; // planar [stream][out_ch][io_stride], nullptr = append only
  long io_stride;
  int n_frames;
  int n_streams, in_ch, out_ch, cols_per_stream;
  int n_cols, cols_pad; // n_streams * cols_per_stream, rounded up to a multiple of kLinearColTile (padded columns stay zero)
  int hist_frames, pos;
  int part_frames; // a multiple of 64, >= n_frames
  int n_splits, split_taps, taps_off;
  float bias;
};
// append + nam_linear_kernel + nam_linear_reduce_kernel (+ zeros for output channels >= cols_per_stream), enqueued on `stream`
hipError_t launch_linear(const LinearArgs& a, hipStream_t stream);

// A SlimmableContainer of Linear models (linear_worklist.h): every stream one column (1-in / 1-out) of the same ring, each on its own
// submodel. One PIECE of a launch, three kernels: nam_linear_append_kernel as above, nam_linear_pairs_kernel over the work list,
// nam_linear_pairs_reduce_kernel (every column sums its own pair's splits and adds that submodel's bias).
struct LinearPairsArgs
{
  // blob: the submodels' padded taps behind one another (LinearPair::taps_off points into it); part: [slab][part_frames][32];
  // n_splits: the grid's split extent (LinearWorkList::grid_splits); split_taps: the largest of the container (the dynamic LDS);
  // in_ch = out_ch = cols_per_stream = 1; taps_off and bias are the pairs'
  LinearArgs a;
  const LinearPair* pairs; // [n_pairs]
  const int32_t* col_pair; // [cols_pad]
  int n_pairs;
  int hist_taps; // the largest n_splits x split_taps of a submodel: the ring keeps that many frames + the piece
};
hipError_t launch_linear_pairs(const LinearPairsArgs& p, hipStream_t stream);

// nam_wn_reg_kernel (plan.h: WrPlan). One launch serves up to kWrMaxGroups WIDTH GROUPS — streams of a slimmable model
// (or container) that currently run different sub-models: workgroups [first, next group's first) belong to group g, each
// with its own op list, weights, LDS layout and state ("LDS repacking" per width); the audio windows are shared.
struct WrGroup
{
  const float* blob; // weights, tables and the op list as the kernel's LDS copy holds them (a multiple of 4 floats)
  float* state; // [stream][state_stride]
  const int* stream_map; // optional: position inside the group -> stream index; nullptr = identity
  long state_stride;
  int n_ops, blob_floats;
  int hist_floats; // floats of ring area behind the positions
  int n_slots; // layers (write positions)
  int tab_rows, n_rows, tab_pf, n_pf, tab_ring, tab_ops; // blob float offsets / entry counts of the tables
  int first; // first workgroup of the group
  int split_op[3]; // pipelined launches: the program's cuts at 1/4, 1/2, 3/4 of its weights (two stages: [1]; four: all three)
  int prog; // per-model code objects with the programs compiled in (NAM_WR_PROGRAMS): which of them this group runs
};
struct WrArgs
{
  WrGroup g[kWrMaxGroups];
  int n_groups;
  const float* in; // nullptr = silence (prewarm)
  float* out; // nullptr = discard
  long io_stride;
  int n_frames;
  int in_ch, out_ch;
  PersistArgs ps;
  // model bank (nam_hip_batch_create_bank; nullptr = one model): a bank launch has ONE group, and stream s runs member
  // m = bank_member[s] (indexed by STREAM, not by launch position) of g[0].blob = [members][bank_stride] floats — whole WrPlan
  // blobs (a multiple of four floats), one layout for every member (api_bank.cpp compares the plans). Read in the prologue, which
  // copies the member's blob to LDS; behind it only the scales of WR_OUTPUT / WR_SET_COND / WR_POST_HEAD ask again (a per-model
  // code object has member 0's compiled in: kernel_wn_reg.hip, wr_op_scale). Behind every other field, as in LSTMArgs.
  const int* bank_member;
  long bank_stride;
};

// stages = 2 / 4: that many wavefronts per stream (the op program cut at WrGroup::split_op), lds_bytes including the
// (stages - 1) queues of kWrQueueBytes
hipError_t launch_wn_reg(const WrArgs& a, int n_workgroups, int lds_bytes, bool layers, bool runs, bool rt_layers, int stages,
                         LaunchStream stream);
// the same kernel compiled for one model's own layer shapes (wr_jit.cpp); fn = hipFunction_t of the model's code object
hipError_t launch_wn_reg_jit(void* fn, const WrArgs& a, int n_workgroups, int lds_bytes, int stages, LaunchStream stream);
hipError_t launch_generic(const GenericArgs& a, int n_blocks, int lds_bytes, hipStream_t stream);
hipError_t launch_a1(const A1Args& a, int n_blocks, hipStream_t stream);
hipError_t launch_a1_mfma(const A1Args& a, int n_blocks, int act, hipStream_t stream);
hipError_t launch_a1_p2(const A1Args& a, int n_blocks, int c0, int c1, int act, LaunchStream stream);
// nam_a1_p4_kernel: the same models as a pipeline of wave sets decoupled through LDS (kernel_a1_p4.hip)
hipError_t launch_a1_p4(const A1Args& a, int n_blocks, int c0, int c1, int act, LaunchStream stream);
hipError_t preload_a1_p4_session(int c0, int c1, int act, bool out_host, bool bank = false); // (kernel_a1_p4.hip)
// nam_a1_q_kernel (kernel_a1_q.hip): the 16 / 8 official topology (aq_table.h) as twelve one-wave stages with LDS-resident
// rings; a.tiles_off = the plan's q weight block (A1Plan::q_w_off), a.consts_off = the FULL-layout tile area (ws_tiles_off)
bool a1_q_takes(int act); // the activations it is compiled for (Fasttanh, Tanh)
hipError_t launch_a1_q(const A1Args& a, int n_blocks, int act, LaunchStream stream);
// nam_kq_kernel (kernel_kq.hip): the A2 topology (kp_table.h) as a pipeline of twelve one-wave stages, one lane per frame, on
// nam_kt_mfma_kernel's stream state; a.tiles_off = the plan's kq weight block (A1Plan::kq_w_off); kq_takes: the activations it
// is compiled for (LeakyReLU with a slope <= 1, ReLU, Tanh, Fasttanh)
bool kq_takes(int act, float act_p0);
hipError_t launch_kq(const A1Args& a, int n_blocks, int act, LaunchStream stream);
hipError_t launch_kt_mfma(const A1Args& a, int n_blocks, int nk, int channels, int lds_aux_floats, int act,
                          hipStream_t stream);
hipError_t launch_lstm(const LSTMArgs& a, hipStream_t stream);
hipError_t launch_lstm_mfma(const LSTMArgs& a, hipStream_t stream);
hipError_t launch_lstm_row(const LSTMArgs& a, LaunchStream stream); // hidden <= 4: one gate row per lane
hipError_t launch_lstm_wide(const LSTMArgs& a, LaunchStream stream); // 5 .. 32 hidden units: two gate rows per lane
int lstm_lds_bytes(const LSTMArgs& a);
long lstm_scratch_floats(const LSTMArgs& a); // > 0: the lanes = streams kernel keeps its columns in global scratch
hipError_t launch_fill_state(float* state, long state_stride, const int* stream_map, int n_streams, const float* init,
                             int n_init, int state_floats, hipStream_t stream);
// the bank form: `init` = [member][n_init], stream s takes row member_of[s] (indexed by STREAM, like LSTMArgs::bank_member)
hipError_t launch_fill_state_bank(float* state, long state_stride, const int* stream_map, int n_streams, const float* init,
                                  const int* member_of, int n_init, int state_floats, hipStream_t stream);
// nam_a2_transcode_kernel (kernel_a2_transcode.hip): the streams `streams` (device memory; nullptr = 0 .. n_streams - 1) of a narrow A2
// container submodel between nam_wn_reg_kernel's state rows (`wr_state`) and the padded rings of the largest submodel's layout
// (`a2_state`), ring by ring of the device table `rings` (a2_transcode.h); a plain copy, zeros into the padded channels
hipError_t launch_a2_transcode(const A2XcRing* rings, int n_rings, float* a2_state, long a2_stride, float* wr_state, long wr_stride,
                               const int* streams, int n_streams, bool to_padded, hipStream_t stream);
// nam_state_rows_copy_kernel (kernel_a2_transcode.hip): the state rows of the streams `streams` (device memory; nullptr = 0 ..
// n_streams - 1) from `src` to `dst`, `floats` floats a row, bit for bit — two allocations that keep one layout
hipError_t launch_state_rows_copy(float* dst, long dst_stride, const float* src, long src_stride, const int* streams, int n_streams, int floats,
                                  hipStream_t stream);
// One stream's columns [col0, col0 + n_cols) of a Linear batch's history ring `hist` = [hist_frames][cols_pad] at position `pos`
// (the row the next frame goes to: the oldest). `rows` = [hist_frames][n_cols] in device memory, oldest frame first
// (stream_state.h: ring_row); unused by LINEAR_COLS_ZERO. No other column is read or written.
enum LinearColsOp : int
{
  LINEAR_COLS_ZERO = 0, // the columns become zero
  LINEAR_COLS_GATHER = 1, // ring -> rows
  LINEAR_COLS_SCATTER = 2 // rows -> ring
};
hipError_t launch_linear_stream_cols(float* hist, int hist_frames, int cols_pad, int pos, int col0, int n_cols, float* rows, LinearColsOp op,
                                     hipStream_t stream);

} // namespace namhip
