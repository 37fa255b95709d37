// api_internal.h — what the translation units behind the C ABI (include/nam_hip.h) share: the model and batch handles, the
// session and ticket records, and the functions they call across files.
//   nam_hip_api.cpp   the extern "C" entry points (argument checks, the order of operations of a call)
//   api_launch.cpp    model -> plans -> device blobs; which kernel a launch runs and its arguments; Reset / prewarm
//   api_session.cpp   persistent block mode: the resident launch, its command ring, completion, the watchdog
//   api_host_io.cpp   host buffers: the windows both sides can reach, blocking calls through a session, tickets
//   api_bank.cpp      model banks: the families' rules (kBankFamily), which models may share a batch, the bank's device image,
//                     per-stream member binding
//   launch_policy.h   nam_wn_reg_kernel's launch shape, workgroups per CU and stream bound: integers in, integers out (no HIP)
//   linear_worklist.h the (column tile, submodel) work list of an all-Linear container's batch: assignment in, tables and extents out (no HIP)
//   a2_transcode.h    an A2 container's narrow submodel between nam_wn_reg_kernel's state and the largest submodel's rings: the table, its check (no HIP)
//   stream_state.h    one stream's state as a blob: header, encode, validate, the Linear ring's row arithmetic (no HIP)
// No exception leaves these files (guarded); errors are codes + nam_hip_last_error.
#pragma once
#include "../../include/nam_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "device_owner.h"
#include "kernels.h"
#include "launch_policy.h"
#include "model_spec.h"
#include "plan.h"
#include "session_command.h"
#include "stream_state.h"
#include "wr_jit.h"

using namespace namhip;

namespace namhip
{
namespace api
{
// the calling thread's last error text (nam_hip_last_error); returns `code`
int fail(int code, const std::string& msg);

#define NAM_HIP_CHECK(expr)                                                                                           \
  do                                                                                                                   \
  {                                                                                                                    \
    hipError_t _e = (expr);                                                                                            \
    if (_e != hipSuccess)                                                                                              \
      return fail(NAM_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));                             \
  } while (0)

template <typename F>
int guarded(F&& f)
{
  try
  {
    return f();
  }
  catch (const FileValidationError& e)
  {
    return fail(NAM_HIP_ERR_FILE, e.what());
  }
  catch (const UnsupportedError& e)
  {
    return fail(NAM_HIP_ERR_UNSUPPORTED, e.what());
  }
  catch (const std::exception& e)
  {
    return fail(NAM_HIP_ERR_MODEL, e.what());
  }
  catch (...)
  {
    return fail(NAM_HIP_ERR_MODEL, "unknown error");
  }
}
} // namespace api
} // namespace namhip
using namespace namhip::api;

struct nam_hip_model
{
  std::shared_ptr<ModelSpec> spec;
  // One plan per distinct width (slimmable WaveNets have several; everything else exactly one).
  std::vector<std::vector<int>> width_channels;
  std::vector<Plan> plans;
  int full_width = 0; // index of the full-size plan
  // A container whose largest submodel is the topology nam_kq_kernel is compiled for and whose other submodels differ from it in
  // channel count only (A2.nam: A2-Lite next to A2-Full; api_launch.cpp: build_model): per narrower submodel a SECOND plan,
  // zero-padded onto the largest one's layout (plan_a1.cpp: build_a2_padded_plan), and the table between the submodel's own
  // nam_wn_reg_kernel state and the padded rings (a2_transcode.h). [submodel]; the largest one's entries stay empty. Both vectors
  // are empty unless EVERY narrower submodel has its pair: a batch at mixed sizes then runs persistent mode as one session.
  std::vector<Plan> padded;
  std::vector<A2Transcode> transcode;
  // Which mixed-size residency a batch of this container has in persistent mode (MixFamily below; MIX_NONE: none, a batch at mixed
  // sizes is a launch per size). MIX_A2: the pair of vectors above is filled. MIX_A1: every submodel is a member of ONE bank of
  // the BANK_A1_IL family (api_bank.cpp: container_a1_difference) — the official topology at (padded) 16 / 8 channels, one
  // activation, one fast_tanh; nothing more is kept, the submodels' own plans are the members. `mix_note`: the sentence
  // NAM_HIP_FIELD_DESCRIPTION says about it ("" for a model the question does not arise for).
  int mix_family = -1;
  std::string mix_note;

  bool slimmable() const { return spec->arch == ARCH_CONTAINER || (spec->arch == ARCH_WAVENET && spec->wavenet.slimmable); }
  int width_for_ratio(double ratio) const
  {
    if (spec->arch == ARCH_CONTAINER)
      return spec->container_index(ratio); // plan i = submodel i
    if (!spec->wavenet.slimmable || spec->arch != ARCH_WAVENET)
      return 0;
    const std::vector<int> ch = channels_for_ratio(spec->wavenet, ratio);
    for (size_t i = 0; i < width_channels.size(); i++)
      if (width_channels[i] == ch)
        return (int)i;
    return -1;
  }
};

// A model bank (nam_hip_bank_create): models that plan onto ONE instantiation of a kernel family — the interleaved-frame kernels
// (nam_a1_q_kernel and its siblings: BANK_A1_IL), the A2 topology's (nam_kq_kernel, nam_kt_mfma_kernel: BANK_A2), the small
// LSTM cells' (nam_lstm_row_kernel, nam_lstm_wide_kernel: BANK_LSTM) or nam_wn_reg_kernel with one program (BANK_WN_REG) — with
// the same blob layout, so that one launch can run
// them side by side, each workgroup on its stream's member. Immutable host data, self-contained (nothing of the member models is
// referenced after creation); a batch created from it shares ownership of `data`, so the handle may be freed while batches live.
enum BankFamily : int
{
  BANK_A1_IL = 0, // the official WaveNet topology at (padded) 16 / 8 channels
  BANK_A2 = 1, // the A2 topology (kp_table.h)
  BANK_LSTM = 2, // LSTMs of one shape on the gate-row kernels (hidden <= 32, one or two layers, one or two inputs)
  BANK_WN_REG = 3, // WaveNets a one-model batch runs on nam_wn_reg_kernel under AUTO (the official nano size, FiLM, gating, a nested
                   // condition_dsp, a post-stack head, narrow plain stacks), of ONE program (WrPlan::structure_key)
  BANK_FAMILY_COUNT
};
struct nam_hip_bank_data
{
  nam_hip_model proto; // member 0's spec and full-size plan (a container member: its largest submodel's): everything a batch asks
                       // its model that is not a weight
  int family = BANK_A1_IL; // decided by member 0 (api_bank.cpp)
  int n_members = 0;
  long blob_stride = 0; // floats per member in `blobs`: the kept part of the plan's blob (api_bank.cpp) rounded up to a multiple of four (16-byte records)
  std::vector<float> blobs; // [n_members][blob_stride]
  // per member besides the blob, at most one of the two (BankFamilyRules::per_member says which; what it does not name stays empty):
  std::vector<float> scal; // [n_members][2]: head_scale, act_p0 (A1Args::bank_scal)
  int n_init = 0; // floats of a member's initial state (LSTMPlan::init_state: h0 / c0 from ITS weight stream)
  std::vector<float> init; // [n_members][n_init]
  // what a stream state blob names its model by (stream_state.h): every member's fingerprint, and the bank's (theirs, in order)
  std::vector<uint64_t> member_fp; // [n_members]
  uint64_t fingerprint = 0;
};
struct nam_hip_bank
{
  std::shared_ptr<const nam_hip_bank_data> data;
};

namespace namhip
{
namespace api
{
static_assert(kCuLdsBytes == kLdsCu, "launch_policy.h counts workgroups per CU with the kernels' LDS size");

// Which layout a WaveNet group's state holds (WidthGroup::state_family; state_family_of, persist_family)
enum StateFamily : int
{
  STATE_FRESH = -1, // freshly zeroed: any layout may follow
  STATE_OPS = 0, // the op program's rings (shared by the A1 kernels unless they run on zero-padded channels: plan.h, Plan::a1_padded_layout)
  STATE_A1_PADDED = 1, // the padded A1 rings
  STATE_WN_REG = 2 // nam_wn_reg_kernel's 64-frame conv-input histories
};

// (every device allocation is an owner, device_owner.h: `g = WidthGroup()` frees the group's, and so does the batch's end)
struct WidthGroup
{
  const Plan* plan = nullptr;
  DeviceBuf<float> d_blob;
  DeviceBuf<NamOp> d_ops;
  DeviceBuf<A1Plan> d_a1;
  DeviceBuf<float> d_wr_blob; // nam_wn_reg_kernel's weights, tables and macro-ops (plan.h: WrPlan)
  DeviceBuf<float> d_state; // [n_streams][state_stride] (allocated when the first stream joins)
  DeviceBuf<float> d_init; // LSTM initial state
  DeviceBuf<float> d_scratch; // LSTM cells too large for LDS: nam_lstm_kernel<true>'s h / c / gate columns
  long scratch_floats = 0;
  long state_stride = 0;
  std::vector<int> streams; // members, ascending
  DeviceBuf<int> d_map; // device copy of `streams` (empty when the group is all streams in order)
  StateFamily state_family = STATE_FRESH; // which layout the state currently holds
  // Prewarm cache (the reference caches what prewarm leaves in every conv, conv1d.cpp:151-161 / model.cpp:737-775, and
  // later Resets refill from it): one stream's state right after zero + prewarm — every stream's is the same — keyed by
  // the kernel that produced it and the frames it ran. A later Reset / SetSlimmableSize copies it instead of running
  // the silence again.
  DeviceBuf<float> d_prewarm;
  int prewarm_kernel = -1, prewarm_len = 0;
  // a bank batch's one group (api_bank.cpp): d_blob holds [members][bank_stride] floats, and the kernels pick a stream's member
  // through d_bank_member[stream] (indexed by STREAM, not by launch position) and its scalars from d_bank_scal[2 member].
  // No prewarm cache: a member's prewarmed state depends on its weights, so a Reset runs the silence for every stream.
  // BANK_MEMBER_INIT_STATES: no d_a1 and no d_bank_scal; d_init holds [members][n_init] floats, a stream's h0 / c0 its member's row.
  // BANK_BLOB_WR: the members' blobs are in d_wr_blob (where pick_kernel and wr_groups look), d_blob stays empty.
  DeviceBuf<int> d_bank_member;
  DeviceBuf<float> d_bank_scal;
  long bank_stride = 0;
  // a Linear batch's one group (plan.h: LinearPlan): no per-stream state — d_state stays empty, state_stride 0 —; the batch's input
  // history as ONE ring [lin_hist_frames][lin_cols_pad], stream-minor, and the K-splits' partial sums of one launch piece
  // [n_splits][lin_part_frames][lin_cols_pad]. d_blob holds the padded taps. `lin_pos`: the ring row the next frame goes to — host
  // state: the launches of a batch are enqueued in call order, each with its position as an argument.
  DeviceBuf<float> d_lin_hist, d_lin_part;
  int lin_hist_frames = 0, lin_cols_pad = 0, lin_part_frames = 0, lin_piece = 0, lin_pos = 0;
};

// A batch of a SlimmableContainer whose submodels are all Linear: the input history does not depend on the impulse
// response, so the batch keeps ONE ring [hist_frames][cols_pad] (column = stream) for all its streams, whichever submodel each is
// on, and a launch piece runs a work list of (column tile, submodel) pairs (linear_worklist.h). The batch's width groups carry the
// submodels' plans and the streams' membership only: no blob, no ring, no state of their own. The tables and `part` are sized at
// creation for the worst assignment; the work list is rebuilt and uploaded by the control calls that change an assignment
// (nam_hip_batch_set_slimmable_size, nam_hip_batch_set_stream_state), never by a process call.
struct LinearContainer
{
  bool on = false;
  std::vector<LinearSub> subs; // [submodel]
  LinearWorkCaps caps;
  LinearWorkList work; // as the device tables hold it
  DeviceBuf<float> d_blob; // the submodels' padded taps behind one another
  DeviceBuf<float> d_hist, d_part; // [hist_frames][cols_pad]; [caps.max_part_slabs][part_frames][32]
  DeviceBuf<LinearPair> d_pairs; // [caps.max_pairs]
  DeviceBuf<int32_t> d_col_pair; // [caps.cols_pad]
  int hist_frames = 0, part_frames = 0, piece = 0;
  int pos = 0; // the ring row the next frame goes to (host state, as WidthGroup::lin_pos)
};

// A batch of a container with a mixed-size residency (nam_hip_model::mix_family) whose streams are at MIXED sizes, in persistent
// mode: the narrow streams live zero-padded in the largest submodel's state rows (`resident`:
// group[full_width].d_state holds EVERY stream's rings; the narrow groups keep their membership, their own rows are stale) and the
// whole batch is one launch of the largest submodel's kernels through their bank path — member = the stream's submodel, member
// full_width = the largest submodel's own blob. Entered and left by control calls only (api_launch.cpp: mix_enter / mix_leave move
// the narrow streams' state); outside persistent mode the batch is never resident and launches per width group as ever.
// The two families differ in their row of kMixFamily and in nothing else:
//  * MIX_A2 (A2.nam: A2-Lite next to A2-Full): nam_kq_kernel / nam_kt_mfma_kernel over the padded plans' WHOLE blobs; a narrow
//    stream's own rows are nam_wn_reg_kernel's layout, so its state moves through a table (nam_a2_transcode_kernel).
//  * MIX_A1 (the official WaveNet topology: standard 16 / 8, lite 12 / 6, feather 8 / 4): the interleaved-frame kernels over the
//    submodels' own blobs from A1Plan::ws_tiles_off on, as a BANK_A1_IL bank batch; a narrow stream's own rows already ARE the
//    padded layout (equal state geometry is part of the bank comparison), so its state moves as a plain row copy
//    (nam_state_rows_copy_kernel).
enum MixFamily : int
{
  MIX_NONE = -1,
  MIX_A2 = 0,
  MIX_A1 = 1,
  MIX_FAMILY_COUNT
};
enum MixMove : int // how a narrow group's rows get into and out of the largest submodel's
{
  MIX_MOVE_TRANSCODE, // ring by ring of nam_hip_model::transcode[submodel] (a2_transcode.h)
  MIX_MOVE_COPY // the whole row as it is
};
struct MixFamilyRules // kMixFamily[MixFamily] (api_launch.cpp); plain data, as BankFamilyRules
{
  const char* name; // as the statistics line and refusals print it
  int persist; // the PersistKind of the one session: what the largest submodel's plan must be eligible for over EVERY stream
  int kernel_class; // the kernel class (NAM_HIP_KERNEL_*) a resident batch's one group runs: the session's and the plain launches'
  int narrow_class; // ... and the class whose state layout a narrow group must keep outside the session (what it runs there)
  unsigned fns; // bit per KernelFn that may launch a resident batch
  const char* launch_refusal; // launch_a1_family's answer to any other function
  int blob_source; // BankBlobSource: what the device image keeps of a submodel's blob, and what the launch arguments are rebased on
  MixMove move;
  const char* mover; // the kernel that moves the rows, as the statistics line names it
};
extern const MixFamilyRules kMixFamily[MIX_FAMILY_COUNT];
struct SizeMix
{
  bool resident = false;
  DeviceBuf<float> d_blob; // [submodel][stride]: what blob_source keeps of every submodel's (padded) plan, the largest one's own at [full_width]
  DeviceBuf<float> d_scal; // [submodel][2]: head_scale, the activation's parameter (A1Args::bank_scal)
  DeviceBuf<int> d_member; // [stream] = nam_hip_batch::stream_width, refreshed whenever the batch becomes resident
  long stride = 0;
  std::vector<DeviceBuf<A2XcRing>> d_rings; // MIX_MOVE_TRANSCODE: [submodel] = nam_hip_model::transcode[submodel].rings
  unsigned long long n_moves = 0; // (NAM_HIP_SESSION_STATS) launches of the family's mover, streams they moved, and the
  unsigned long long n_streams_moved = 0; // host's time in them, the wait for the batch's stream included
  double t_move_us = 0;
};

// Persistent block mode (nam_hip_batch_set_persistent): one resident launch of nam_a1_p2_kernel per session, fed one
// command per 64-frame buffer through a device-memory ring (kernel_a1_p2.hip, PERSIST).
constexpr unsigned kPRing = 1024; // commands in flight at most (power of two)
// behind the ring: d_ring[kPRing] = the "leave" word of sessions whose launch lingers (ticketed host buffers: A1Args::p_linger) —
// the host stores the session's command count there when it wants the launch gone (a flush, the end of the session): a
// workgroup that has consumed exactly that many commands and finds no next one leaves at once instead of lingering
constexpr unsigned kPRingTail = 8;
constexpr int kTicketLingerDefault = 20000; // 200 us of the 100 MHz clock: workgroups drift apart by up to NAM_HIP_PIPE_SLOTS buffers (16 x 5.3 us) —
                                     // the one in front must outwait the host, which hands the next buffer in when the LAST one has finished an old one
// (NAM_HIP_TICKET_LINGER_US overrides it; 0 or 1: a ticket session's launch leaves as promptly as any other — for hosts that run several
// sessions on one device, where a lingering launch of one holds the CUs the other's launch is waiting for)
inline int ticket_linger_from_env() // (read when a batch is created, like the other switches)
{
  const char* e = std::getenv("NAM_HIP_TICKET_LINGER_US");
  return e ? (int)std::min(std::max(std::atol(e), 0l), 100000l) * 100 : kTicketLingerDefault;
}
struct PersistSession
{
  bool enabled = false; // the caller opted in
  bool active = false; // a window is registered; a launch of the session may be consuming commands
  // the command ring: (seq << 32) | frame offset, in FINE-GRAINED device memory — local to the workgroups that poll
  // it, and host-writable through the PCIe BAR (MI355X exposes all of HBM): the host stores a command itself when the
  // caller's stream is idle (the usual real-time case: nothing to order behind; a posted write, ~0.1 us), else the
  // store is enqueued on that stream (hipStreamWriteValue64: ~4 us of host time and a small kernel on the device)
  DeviceBuf<unsigned long long> d_ring;
  bool host_store_ok = false; // the ring is fine-grained memory (else plain device memory: stream-ordered stores only)
  MappedBuf<unsigned> words; // host-mapped: [0, n_wg) progress, [n_wg, 2 n_wg) completion (bit 31 = exited); host() / dev(): the same words as either side sees them
  DeviceBuf<unsigned> d_cons; // device memory: commands consumed per workgroup (where its next launch resumes)
  DeviceBuf<unsigned> d_cmd_count; // device memory [kPRing]: workgroups through command c (A1Args::p_cmd_count), zero between commands
  MappedBuf<unsigned> cmd_done; // host-mapped [kPRing]: c + 1 once every workgroup is through command c
  hipStream_t last_caller = nullptr; // the stream the last doorbell was rung on (the caller's: not owned)
  int grace = 0; // A1Args::p_grace of the next launch
  long long seq0 = -1; // A1Args::p_seq0 / p_cmd0 of the next launch
  unsigned long long cmd0 = 0;
  unsigned flushed = 0; // every workgroup has consumed exactly this many commands (valid while == seq)
  bool flushed_valid = false;
  bool outstanding = false; // a launch of the session may still be running
  bool need_order = false; // the next launch must wait for the batch's own stream (session start)
  StreamOwner kstream; // the resident launch's own stream (nothing else may be enqueued behind it)
  EventOwner order; // makes the launch wait for what the caller had enqueued before the first buffer
  unsigned seq = 0; // commands submitted in this session
  const float* in_base = nullptr;
  float* out_base = nullptr;
  bool out_is_host = false; // the output window is host memory (A1Args::p_out_host)
  long stride = 0;
  int n_wg = 0; // workgroups of the session's launch
  int kind = -1; // PersistKind
  int done_off = 0; // words: [0, done_off) progress words, [done_off, 2 done_off) completion words
  // Sequence numbers are 31-bit (bit 31 of a completion word is the "left" flag): a session START — where every
  // workgroup stands at exactly `seq` and nothing is in flight — rebases them to 0 once they pass this mark
  // (NAM_HIP_PERSIST_REBASE_AT overrides it: tests)
  unsigned rebase_at = 0x40000000u;
  bool prepared = false; // persist_prepare ran to its end (every window-independent resource is there)
  bool rebase_pending = false; // persist_submit ended the session because the next buffer would cross the rebase mark: persist_start renumbers
  long timeout_ms = 20000; // a resident launch that makes no progress for this long is a device failure (NAM_HIP_PERSIST_TIMEOUT_MS)
  // developer statistics (NAM_HIP_SESSION_STATS=1: printed when the batch is destroyed)
  unsigned long long n_launches = 0, n_host_doorbells = 0, n_stream_doorbells = 0, n_starts = 0, n_flush_relaunches = 0;
  double t_poll = 0, t_out = 0, t_in = 0, t_cmd = 0, t_poll_max = 0, t_out_max = 0, t_in_max = 0, t_cmd_max = 0; // us (NAM_HIP_SESSION_STATS)
  MappedBuf<long long> why; // (NAM_HIP_SESSION_STATS) per workgroup: reason << 56 | grace loop << 48 | all-through count << 24 | own count
  unsigned long long n_waits = 0, n_polls = 0; // ticket waits, looks at the buffer's completion word
  unsigned long long n_publishing = 0, n_lingering = 0; // launches that publish every command; those of them that linger for the next one
  unsigned epoch = 0; // counts session starts (a ticket of an earlier session is complete: sessions end flushed)
  // Burst lengths (commands between two whole flushes) of this session, newest first; ~0u = not seen yet. A host that flushes after
  // every buffer or two (a device-resident real-time chain: process_device + flush per 64 .. 256 frames) waits for the FIRST buffer of
  // every launch: the official 16 / 8 topology then starts as nam_a1_p4_kernel (four waves per layer: the first buffer is through in
  // ~6 us) instead of nam_a1_q_kernel (one wave per layer: ~27 us, faster only once buffers overlap) — the rule of the blocking host
  // calls (CallHints::short_blocking_call), learnt from the caller's own pattern: three bursts in a row of at most four buffers
  unsigned bursts[3] = {~0u, ~0u, ~0u};
  unsigned burst_start = 0; // `seq` at the last whole flush
  bool short_bursts() const { return bursts[0] <= 4u && bursts[1] <= 4u && bursts[2] <= 4u; }
  bool one_buffer_bursts() const { return bursts[0] == 1u && bursts[1] == 1u && bursts[2] == 1u; } // (nam_wn_reg_kernel: one wave per stream then)
  EventOwner retired; // the completion signal of the session's latest launch (kernels.h: LaunchStream), recorded by the dispatch itself
  bool cmd_done_published = false; // the running launch stores p_cmd_done behind every command's results (A1Args::p_out_host == 2; PersistArgs::cmd_done); p_prog stays ring bookkeeping every 16 commands
  bool all_resident = false; // every workgroup of the latest launch is on the chip at once (persist_launch; session_lingers): it need not take turns
};

// One buffer in flight between nam_hip_batch_submit_f32 and nam_hip_batch_wait_f32
struct PipeSlot
{
  long long ticket = -1;
  bool in_flight = false;
  int n_frames = 0;
  int how = 0; // 0: a command range of the host-mapped session | 1: copies + launch on the batch's stream, `done` behind them | 2: rendered by a blocking call, kept in `held`
  unsigned seq_end = 0, epoch = 0; // how == 0: the session's command count behind this buffer, the session it belongs to
  EventOwner done;
  std::vector<float> held;
};

// The two windows of host buffers a session reads and writes itself (api_host_io.cpp: host_windows): both or neither
struct HostWindows
{
  DeviceBuf<float> in_bar; // one address for both sides
  MappedBuf<float> out_map; // host() / dev(): the host's address / the same memory as the device sees it
  bool failed = false; // the allocation was refused once: the copying path stays
};
} // namespace api
} // namespace namhip

struct nam_hip_batch
{
  const nam_hip_model* model = nullptr; // (a bank batch: &bank->proto)
  std::shared_ptr<const nam_hip_bank_data> bank; // nam_hip_batch_create_bank; nullptr = one model
  std::vector<int> stream_member; // bank batches: member of every stream
  int device = 0;
  int n_streams = 0;
  int max_frames = 0;
  // Release order = the members' declaration order, backwards (nam_hip_batch_destroy only quiesces and deletes): the session (`ps`,
  // the last owner below) goes first, then the groups, then staging and windows, then the ticket events (`pipe`), and `stream`
  // last, when nothing that was enqueued on it is left. A new owner goes where its release belongs in that order.
  StreamOwner stream;
  PipeSlot pipe[NAM_HIP_PIPE_SLOTS];
  DeviceBuf<float> d_in; // staging for the host-pointer entry points
  DeviceBuf<float> d_out;
  PinnedBuf<float> h_stage; // pinned, used by the f64 path
  // host-mapped staging of the blocking entry points in persistent mode: the session's kernel reads the input from and
  // writes the output to host memory itself (its input loads / output stores are system-scope anyway), so a blocking
  // call is: copy in, store the command(s), watch the completion words, copy out — no launch of a copy, no stream sync
  // input: FINE-GRAINED DEVICE memory the host writes through the PCIe BAR (posted writes; the device then reads local
  // HBM — device reads of host memory serialise at a microsecond or two per wavefront: 1.9 ms per buffer at 256 streams);
  // output: host-mapped memory the device writes (posted writes again), read by the host from its own DRAM
  HostWindows win;
  // the ticketed entry points (nam_hip_batch_submit_f32) have windows of their own, the same two kinds of memory,
  // NAM_HIP_PIPE_SLOTS buffers deep: [slot][row][max_frames], slot = ticket % NAM_HIP_PIPE_SLOTS
  HostWindows pipe_win;
  long long pipe_next = 0; // the next ticket
  bool pipe_session = false; // the session serves ticketed buffers: its launches publish every command (PersistSession::cmd_done_published)
  PinnedBuf<float> pipe_h_in, pipe_h_out; // staging of the copying form ([slot][row][max_frames])
  DeviceBuf<float> pipe_d_in, pipe_d_out;
  std::vector<float> pipe_cvt; // the _f64 forms of submit / wait: one buffer of float32 on the way in / out
  int kernel = NAM_HIP_KERNEL_AUTO;
  std::vector<WidthGroup> groups;
  SizeMix mix; // (mix.resident: a container's batch at mixed sizes in persistent mode, one session)
  LinearContainer lin; // (lin.on: an all-Linear container's batch)
  std::vector<int> stream_width;
  bool was_reset = false;
  bool reset_with_prewarm = true; // thread_local gPrewarmOnResetDefault = true (NAM/dsp.cpp:20)
  // the caller-supplied stream of the last nam_hip_batch_process_device: control calls that free or rewrite device
  // memory (Reset, SetSlimmableSize, destroy) wait for it as well as for the batch's own stream
  hipStream_t last_ext_stream = nullptr; // (the caller's: not owned)
  int wr_last_stages = 0; // (NAM_HIP_SESSION_STATS: what nam_wn_reg_kernel's last multi-buffer launch ran as)
  bool wr_last_dense = false;
  bool blocking_linger = false; // blocking host calls are coming back to back (the previous one returned < kBlockingLingerGapUs ago): the session's
                                // launch publishes every command and lingers for the next call, like a ticket session's
  double t_blocking_return = -1e18; // host clock (us) when the last blocking host call of the session path returned
  int blocking_linger_us = 200; // 0 = blocking host calls never make a launch linger (NAM_HIP_BLOCKING_LINGER_US)
  int blocking_linger_gap_us = 50; // "back to back": the previous blocking call returned less than this ago
  int ticket_linger = kTicketLingerDefault; // ticks of the 100 MHz clock a ticket session's launch looks for the next buffer (NAM_HIP_TICKET_LINGER_US)
  // NAM_HIP_MAX_STAGES = 1 / 2 / 4 (developer switch; default: no cap): the most pipeline stages a stream is spread over.
  // 1 = no pipelines at all (`no_pipe`: nam_a1_p2_kernel where nam_a1_p4 / q would run, nam_kt_mfma_kernel instead of nam_kq_kernel,
  // nam_wn_reg_kernel as one wavefront per stream — the A/B and reference renderings of the tests); 2 / 4 cap nam_wn_reg_kernel's
  // wavefronts per stream (the compile-time pipelines have fixed stage counts)
  int wr_max_stages = 4;
  bool no_pipe = false;
  PersistSession ps;
  int n_cus = 0; // compute units of the device
};


namespace namhip
{
namespace api
{
// which kernel family a persistent session of a batch runs (api_session.cpp: persist_kind)
enum PersistKind : int
{
  PERSIST_NONE = -1,
  PERSIST_A1_P2 = 0, // nam_a1_q_kernel / nam_a1_p4_kernel (nam_a1_p2_kernel with NAM_HIP_MAX_STAGES=1): one workgroup (most of a CU's LDS) per stream
  PERSIST_WN_REG = 1, // nam_wn_reg_kernel: one wavefront per stream
  PERSIST_LSTM_ROW = 2, // nam_lstm_row_kernel: one wavefront per four streams
  PERSIST_LSTM_WIDE = 3, // nam_lstm_wide_kernel: one wavefront per stream
  PERSIST_KQ = 4 // nam_kq_kernel (the A2 topology): one workgroup (most of a CU's LDS) per stream, as PERSIST_A1_P2
};

// (kPersistTurns, how many turns a session's workgroups may take on the chip: launch_policy.h)
constexpr int kGraceUs = 40; // how long a fresh launch looks for the doorbell it was started for
constexpr int kPersistMaxFrames = 2048; // buffers up to this long go through the session as ceil(n_frames / 64) commands
static_assert(session::kCmdFrames == kBlock, "a whole session command is one device block");
// Session kernels that take a frame count with every command (PersistWave hands it out: persist_wave.h), so a call of ANY length up to
// kPersistMaxFrames stays in the session. The pipeline kernels (PERSIST_A1_P2, PERSIST_KQ) hand fixed sub-blocks from stage to stage:
// their sessions take multiples of 64 frames only, any other length ends the session and runs a plain launch.
constexpr bool persist_any_length(int kind)
{
  return kind == PERSIST_WN_REG || kind == PERSIST_LSTM_ROW || kind == PERSIST_LSTM_WIDE;
}

// The non-empty groups of a batch when ALL of them run nam_wn_reg_kernel (then one launch serves the whole batch, and a
// persistent session can too); n = 0 otherwise. (A fixed array: this runs inside process calls, which allocate nothing.)
struct WrGroupList
{
  WidthGroup* g[kWrMaxGroups];
  int n = 0;
};

// Every __global__ function a group's launch can run. The public NAM_HIP_KERNEL_* values (include/nam_hip.h) name what a caller
// may force, and pick_kernel / kernel_for_launch the family a group runs (the prewarm cache and the state layout key on those);
// which function of the family a launch runs also depends on the launch: select_kernel.
enum KernelFn : int
{
  FN_GENERIC, FN_WN_REG, FN_A1, FN_A1_MFMA, FN_KT_MFMA, FN_KQ, FN_A1_P2, FN_A1_P4, FN_A1_Q, // WaveNets
  FN_LSTM, FN_LSTM_MFMA, FN_LSTM_MFMA_REG, FN_LSTM_ROW, FN_LSTM_WIDE,
  FN_LINEAR, // (the compute kernel of a Linear launch piece; its append and reduce kernels ride along: kernel_linear.hip)
  KERNEL_FN_COUNT
};
// A bank family's rules: kBankFamily[BankFamily] (api_bank.cpp), asked by pick_kernel, launch_a1_family and
// nam_hip_batch_set_kernel. A new family adds an enumerator, a row, its branch of member_refusal and its comparison (api_bank.cpp);
// no other file names a family. Plain data: a const table is compiled for the device too, where no host function can be pointed at.
enum BankBlobSource : int // which part of which of a member's blobs the bank keeps
{
  BANK_BLOB_KERNEL_REGION, // Plan::blob from A1Plan::ws_tiles_off on (bank_blob_base)
  BANK_BLOB_WHOLE, // Plan::blob whole, base offset 0
  BANK_BLOB_WR // Plan::wr.blob whole, base offset 0 (nam_wn_reg_kernel's weights, tables and program)
};
enum BankPerMember : int // what a member carries besides its blob
{
  BANK_MEMBER_SCALARS, // two scalars (nam_hip_bank_data::scal: head_scale, act_p0) and the device A1Plan of member 0
  BANK_MEMBER_INIT_STATES, // its initial state (nam_hip_bank_data::init)
  BANK_MEMBER_NOTHING // everything is in the blob
};
struct BankFamilyRules
{
  const char* name; // as refusals print it
  // the kernel class (NAM_HIP_KERNEL_*) pick_kernel answers for a bank group, which is also the one explicit choice
  // nam_hip_batch_set_kernel admits besides AUTO; NAM_HIP_KERNEL_AUTO: neither (no WaveNet group: select_kernel answers for it)
  int kernel_class;
  const char* set_kernel_refusal; // nam_hip_batch_set_kernel's answer to any other choice
  unsigned fns; // bit per KernelFn that may run a bank group
  const char* launch_refusal; // launch_a1_family's answer to any other function
  BankBlobSource blob_source; // what the bank keeps of a member (bank_blob, bank_blob_base)
  BankPerMember per_member;
};
extern const BankFamilyRules kBankFamily[BANK_FAMILY_COUNT];
inline const BankFamilyRules& bank_rules(const nam_hip_batch* b) // (b->bank is set: a bank batch)
{
  return kBankFamily[b->bank->family];
}
// first float of a member's blob the bank keeps (the single copy: nam_hip_bank_create cuts there, launch_a1_family rebases on it)
int bank_blob_base(const Plan& p, int family);
// the blob of a member's plan the family's kernels read (BankFamilyRules::blob_source)
const std::vector<float>& bank_blob(const Plan& p, int family);

// What a blocking host call knows about itself (process_host_mapped); every other API call has none
struct CallHints
{
  bool short_blocking_call = false; // up to four buffers and the caller waits: the FIRST buffer's latency counts — nam_a1_p4_kernel (~6 us through the model), not nam_a1_q_kernel (~30 us; faster once buffers overlap)
  bool one_buffer_call = false; // ONE 64-frame buffer: nothing to overlap, a launch started now runs nam_wn_reg_kernel as one wave per stream
};
// What a launch is for: built where the API call knows the facts, handed down by const&, stored nowhere. Default: an ordinary launch.
struct LaunchContext
{
  int session_kind = PERSIST_NONE; // PersistKind of the session whose resident launch this is (persist_launch)
  CallHints hints; // of the API call the launch is started for
  hipEvent_t retired = nullptr; // a resident launch: the session's completion event (PersistSession::retired; kernels.h: LaunchStream)
  long long* dbg = nullptr; // nam_hip_batch_debug_timeline: the profiling instantiation's device buffer
};
// The API call a session function works for: the stream its doorbells are rung on (not owned), and its hints for a launch the function starts
struct SessionCaller // (a bare stream: a caller without hints)
{
  hipStream_t stream;
  CallHints hints;
  SessionCaller(hipStream_t s, CallHints h = CallHints()) : stream(s), hints(h) {}
};

// api_launch.cpp
int upload_group(nam_hip_batch* b, WidthGroup& g);
int ensure_state(nam_hip_batch* b, WidthGroup& g);
hipError_t quiesce(nam_hip_batch* b);
StateFamily state_family_of(const Plan& p, int kernel);
int refresh_map(nam_hip_batch* b, WidthGroup& g);
int pick_kernel(const nam_hip_batch* b, const WidthGroup& g);
const char* group_kernel_name(const nam_hip_batch* b, const WidthGroup& g, int n_frames);
PersistArgs persist_args(const nam_hip_batch* b, const LaunchContext& ctx);
int launch_wr(nam_hip_batch* b, WidthGroup* const* groups, const int* const* maps, const int* counts, int n_groups,
              const float* d_in, float* d_out, int n_frames, long io_stride, hipStream_t s, const LaunchContext& ctx);
WrGroupList wr_groups(nam_hip_batch* b);
int launch_wr_all(nam_hip_batch* b, const WrGroupList& gs, const float* d_in, float* d_out, int n_frames, long io_stride,
                  hipStream_t s, const LaunchContext& ctx);
bool wr_session_all_resident(nam_hip_batch* b, const WrGroupList& gs, const LaunchContext& ctx);
int kernel_for_launch(const nam_hip_batch* b, const WidthGroup& g, int n_frames);
int launch_group(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n, const float* d_in, float* d_out,
                 int n_frames, long io_stride, hipStream_t s, const LaunchContext& ctx);
int prewarm_frames(const nam_hip_batch* b, const Plan& p);
int reset_streams(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n, bool prewarm, int first_stream);
// fresh state for the streams `moved` (ascending, not empty) that have just joined `g`: their ids to the device, optionally their
// members' initial states (an LSTM bank), Reset (+ prewarm as the batch was last reset), and the batch's stream drained
int reset_moved_streams(nam_hip_batch* b, WidthGroup& g, const std::vector<int>& moved, bool fill_initial_states);
// a control call's stream list as ascending unique ids (stream_ids == nullptr: every stream); an id out of range fails as `who`
int collect_stream_ids(const nam_hip_batch* b, const int* stream_ids, int n_ids, const char* who, std::vector<int>& ids);
// the streams `moved` (ascending) leave their width groups for group `w`: membership, the group's state allocation, every group's
// device map. Their state in `w` is whatever lies there: the caller resets or writes it. The batch is quiesced.
int move_streams_to_width(nam_hip_batch* b, const std::vector<int>& moved, int w);
// An all-Linear container's batch (LinearContainer). lin_container_model: the model is one. _create: the ring, the tables and the
// first work list, every stream on the last submodel. _launch: a launch of any length, cut into pieces. _move: the streams `moved`
// (ascending) go to submodel `w` — membership, optionally their columns zeroed over the whole ring, the work list rebuilt and
// uploaded; the batch is quiesced, and its stream is drained on return.
bool lin_container_model(const nam_hip_model& m);
int lin_container_create(nam_hip_batch* b);
int lin_container_launch(nam_hip_batch* b, const float* d_in, float* d_out, int n_frames, long io_stride, hipStream_t s);
int lin_container_move(nam_hip_batch* b, const std::vector<int>& moved, int w, bool zero_columns);
// frames of history one stream of such a batch keeps at this max_frames
int lin_container_hist_frames(const nam_hip_model& m, int max_frames);
// Stream slots (include/nam_hip.h: nam_hip_batch_restart_streams, _get / _set_stream_state), behind the entry points' argument
// checks. Each quiesces the batch first and leaves its stream drained.
// `ids`: ascending, unique, in range. The state of a newly created batch after nam_hip_batch_reset(prewarm) for these streams.
int restart_streams(nam_hip_batch* b, const std::vector<int>& ids, bool prewarm);
int64_t stream_state_bytes(const nam_hip_batch* b, int stream);
int get_stream_state(nam_hip_batch* b, int stream, void* buf); // (buf: stream_state_bytes(b, stream) bytes)
int set_stream_state(nam_hip_batch* b, int stream, const void* buf, int64_t size);
// 64 bits that name a model: architecture, config text, fast_tanh and weights (a container: its submodels'; a nested condition_dsp's too)
uint64_t model_fingerprint(const ModelSpec& s);
// A container's batch at mixed sizes (SizeMix). _wanted: persistent mode is on, more than one size is in use, and a session of the
// family's kernels over the device image can hold the batch. _enter / _leave: the narrow streams' state into / out of the largest
// submodel's rows (the family's mover; the batch is quiesced by them, its stream drained on return); no-ops when the batch is
// already there. _sync: whichever of the two `_wanted` asks for — the last step of every control call that changes a size, the
// mode, the kernel choice or a stream's state; such a call starts with _leave, so between the two the batch is what it is
// outside persistent mode.
bool mix_wanted(const nam_hip_batch* b);
int mix_enter(nam_hip_batch* b);
int mix_leave(nam_hip_batch* b);
int mix_sync(nam_hip_batch* b);
inline const MixFamilyRules& mix_rules(const nam_hip_batch* b) // (b->model->mix_family is one: mix.resident says so)
{
  return kMixFamily[b->model->mix_family];
}
// whether a launch or a session of the batch touches the group's own state rows (a resident batch: the largest submodel's only)
inline bool group_state_in_play(const nam_hip_batch* b, const WidthGroup& g)
{
  return !g.streams.empty() && (!b->mix.resident || &g == &b->groups[(size_t)b->model->full_width]);
}
// api_session.cpp
StateFamily persist_family(const nam_hip_batch* b, const WidthGroup& g);
int persist_kind(const nam_hip_batch* b);
// the session a WaveNet group's plan is eligible for if the group held every stream of the batch (persist_kind's rule; mix_wanted
// asks it of the largest submodel)
int wavenet_persist_kind(const nam_hip_batch* b, const WidthGroup& g);
int persist_flush(nam_hip_batch* b, const SessionCaller& caller);
int persist_wait(nam_hip_batch* b, const SessionCaller& caller, unsigned target, bool whole);
int persist_stop(nam_hip_batch* b, CallHints hints);
int persist_prepare(nam_hip_batch* b);
int persist_start(nam_hip_batch* b, const float* d_in, float* d_out, long stride);
int persist_submit(nam_hip_batch* b, const float* d_in, float* d_out, int n_frames, long stride, const SessionCaller& caller);
int persist_submit_block(nam_hip_batch* b, const float* d_in, float* d_out, long stride, const SessionCaller& caller, int n = kBlock);
void persist_free(nam_hip_batch* b);
// api_launch.cpp
int build_model(std::shared_ptr<ModelSpec> spec, nam_hip_model** out);
// api_bank.cpp
int upload_bank_group(nam_hip_batch* b, WidthGroup& g);
int bank_fill_initial_state(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n);
int bank_set_stream_model(nam_hip_batch* b, const int* stream_ids, int n_ids, int member);
// Whether a container's submodels are members of ONE bank of the BANK_A1_IL family with the largest one as member 0 — member_refusal
// and the family's comparison, the ones nam_hip_bank_create runs. "" = they are; else the first reason, naming the submodel.
std::string container_a1_difference(const nam_hip_model& m);
// api_host_io.cpp
bool host_windows(nam_hip_batch* b, int slots, HostWindows& w, bool prealloc = false);
bool host_mapped_applies(nam_hip_batch* b, int n_frames);
int process_host_mapped(nam_hip_batch* b, const float* in_f32, const double* in_f64, float* out_f32, double* out_f64, int n_frames);
int pipe_submit(nam_hip_batch* b, const float* in, int n_frames, PipeSlot& sl, int slot);
int pipe_wait(nam_hip_batch* b, PipeSlot& sl, int slot, float* out);

inline bool persist_eligible(const nam_hip_batch* b)
{
  return persist_kind(b) != PERSIST_NONE;
}

// the official 16 / 8 topology's pipeline: nam_a1_q_kernel (one-wave stages, LDS-resident rings) for the activations it is compiled
// for, nam_a1_p4_kernel otherwise (and for the other official sizes)
inline bool q_runs(const nam_hip_batch*, const Plan& p)
{
  return p.a1.q_ok && a1_q_takes(p.a1.arr[0].act);
}

// the A2 topology's pipeline: nam_kq_kernel (one lane per frame, 4x4x1 matrix instructions) for the activations it is compiled
// for (kernel_kq.hip: kq_takes); any other activation on that topology has no pipeline: nam_kt_mfma_kernel, a launch per buffer
inline bool kq_runs(const nam_hip_batch*, const Plan& p)
{
  return p.a1.kp_ok && kq_takes(p.a1.arr[0].act, p.a1.arr[0].act_p0);
}

// how long a session's launch that publishes every command looks for the next one (ticks of the 100 MHz clock)
inline int session_linger_ticks(const nam_hip_batch* b)
{
  return (b->blocking_linger && !b->pipe_session) ? b->blocking_linger_us * 100 : b->ticket_linger;
}

// Whether the session's running launch lingers for the next command instead of leaving when the ring is empty (A1Args::p_linger):
// it publishes every command, the host can store its "leave" word itself, and every workgroup is on the chip at once (more
// workgroups than CUs take turns: the ones on the chip must leave when the ring is empty). The host and the resident kernel must agree.
// PersistSession::all_resident is persist_launch's answer for the launch it started: one workgroup per CU for the pipeline kernels,
// launch_policy.h: launch_all_resident for nam_wn_reg_kernel (the wavefront form actually launched) and the two LSTM kernels.
inline bool session_lingers(const nam_hip_batch* b)
{
  return b->ps.cmd_done_published && b->ps.host_store_ok && b->ps.all_resident;
}

inline double stat_now_us()
{
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline bool stats_on()
{
  static const bool on = [] { const char* e = std::getenv("NAM_HIP_SESSION_STATS"); return e && e[0] == '1'; }();
  return on;
}

// A row of audio into the PCIe window. Non-temporal stores: the window is write-combining memory, where glibc's memcpy
// (rep movsb from a few KB up) moves 8 GB/s and 16-byte streaming stores 40 (tools/src/host_window_copy.hip,
// profiles/r04/host_window_copy.txt).
inline void copy_to_window(float* dst, const float* src, size_t n)
{
#if defined(__x86_64__)
  size_t i = 0;
  while (i < n && (reinterpret_cast<uintptr_t>(dst + i) & 15u) != 0)
  {
    dst[i] = src[i];
    i++;
  }
  typedef float v4f __attribute__((vector_size(16)));
  typedef float v4f_u __attribute__((vector_size(16), aligned(4)));
  for (; i + 4 <= n; i += 4)
    __builtin_nontemporal_store(*reinterpret_cast<const v4f_u*>(src + i), reinterpret_cast<v4f*>(dst + i));
  for (; i < n; i++)
    dst[i] = src[i];
#else
  std::memcpy(dst, src, n * sizeof(float));
#endif
}

inline void push_out_host_stores()
{
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_sfence(); // (write-combining stores through the BAR: out before the command that points at them)
#else
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}

} // namespace api
} // namespace namhip
