// api_launch.cpp — model handles -> plans -> device blobs; which kernel a launch of a width group runs and its arguments;
// Reset / prewarm (NAM/dsp.cpp:67-140); stream slots (restart one stream, its state out of and into a batch). See api_internal.h.
#include "api_internal.h"

namespace namhip
{
namespace api
{

int upload_group(nam_hip_batch* b, WidthGroup& g)
{
  const Plan& p = *g.plan;
  NAM_HIP_CHECK(upload(g.d_blob, p.blob.data(), p.blob.size(), 1));
  if (p.arch == ARCH_WAVENET)
  {
    NAM_HIP_CHECK(upload(g.d_ops, p.ops.data(), p.ops.size()));
    if (p.a1.valid)
      NAM_HIP_CHECK(upload(g.d_a1, &p.a1, 1));
    if (p.wr.ok)
      NAM_HIP_CHECK(upload(g.d_wr_blob, p.wr.blob.data(), p.wr.blob.size()));
  }
  else if (p.arch == ARCH_LSTM)
    NAM_HIP_CHECK(upload(g.d_init, p.lstm.init_state.data(), p.lstm.init_state.size(), 1));
  else if (p.arch == ARCH_LINEAR)
  {
    // no per-stream state: the geometry of the batch's history ring and partial sums (ensure_state allocates them)
    const LinearPlan& L = p.linear;
    const long cols = (long)b->n_streams * L.cols_per_stream;
    if (cols > (1l << 24))
      return fail(NAM_HIP_ERR_UNSUPPORTED, "Linear: more than 16,777,216 columns (streams x channels) in one batch");
    g.lin_cols_pad = (int)((cols + kLinearColTile - 1) / kLinearColTile * kLinearColTile);
    g.lin_piece = L.piece_frames(b->max_frames);
    g.lin_part_frames = (g.lin_piece + kBlock - 1) / kBlock * kBlock;
    g.lin_hist_frames = L.hist_frames(b->max_frames);
    g.lin_pos = 0;
    g.state_stride = 0;
    return NAM_HIP_OK;
  }
  g.state_stride = p.state_floats;
  return NAM_HIP_OK;
}

int ensure_state(nam_hip_batch* b, WidthGroup& g)
{
  if (g.plan->arch == ARCH_LINEAR)
  {
    if (g.d_lin_hist)
      return NAM_HIP_OK;
    const size_t hist_bytes = (size_t)g.lin_hist_frames * g.lin_cols_pad * sizeof(float);
    NAM_HIP_CHECK(hipMalloc(g.d_lin_hist.out(), hist_bytes));
    NAM_HIP_CHECK(hipMalloc(g.d_lin_part.out(), (size_t)g.plan->linear.n_splits * g.lin_part_frames * g.lin_cols_pad * sizeof(float)));
    NAM_HIP_CHECK(hipMemsetAsync(g.d_lin_hist.get(), 0, hist_bytes, b->stream.get())); // history starts at zero (Buffer, dsp.cpp:203-230)
    g.lin_pos = 0;
    return NAM_HIP_OK;
  }
  if (g.d_state)
    return NAM_HIP_OK;
  const size_t bytes = (size_t)b->n_streams * g.state_stride * sizeof(float);
  NAM_HIP_CHECK(hipMalloc(g.d_state.out(), bytes));
  NAM_HIP_CHECK(hipMemsetAsync(g.d_state.get(), 0, bytes, b->stream.get()));
  if (g.plan->arch == ARCH_LSTM && g.d_bank_member) // a bank: every stream its member's h0 / c0
    return bank_fill_initial_state(b, g, nullptr, b->n_streams);
  if (g.plan->arch == ARCH_LSTM) // h0 / c0 from the weight stream, once per (sub)model instance (lstm.cpp:24-28)
    NAM_HIP_CHECK(launch_fill_state(g.d_state.get(), g.state_stride, nullptr, b->n_streams, g.d_init.get(),
                                    (int)g.plan->lstm.init_state.size(), g.plan->state_floats, b->stream.get()));
  return NAM_HIP_OK;
}

// Wait for everything the batch may still have in flight: its own stream and the last caller-supplied one.
hipError_t quiesce(nam_hip_batch* b)
{
  if (b->ps.active && persist_stop(b, CallHints()) != NAM_HIP_OK) // a resident launch owns the streams' state until it has left
    return hipErrorUnknown;
  hipError_t e = b->stream ? hipStreamSynchronize(b->stream.get()) : hipSuccess;
  if (b->last_ext_stream && b->last_ext_stream != b->stream.get())
  {
    const hipError_t e2 = hipStreamSynchronize(b->last_ext_stream);
    if (e == hipSuccess)
      e = e2;
  }
  return e;
}

StateFamily state_family_of(const Plan& p, int kernel)
{
  if (kernel == NAM_HIP_KERNEL_WN_REG)
    return STATE_WN_REG;
  return (p.a1_padded_layout && kernel != NAM_HIP_KERNEL_GENERIC) ? STATE_A1_PADDED : STATE_OPS;
}

// The op program, the A1 kernels of a channel-padded model and nam_wn_reg_kernel keep different ring layouts: a launch that would
// run `fam` on state of another one is refused — a change of kernel family is only legal on freshly reset state — else the state is `fam`'s
static int claim_state_family(WidthGroup& g, StateFamily fam)
{
  if (g.state_family != STATE_FRESH && g.state_family != fam)
    return fail(NAM_HIP_ERR_INVALID_ARGUMENT,
                "kernel change crosses state layouts (the op program's rings, the A1 kernels' zero-padded rings and "
                "nam_wn_reg_kernel's conv-input histories differ): call nam_hip_batch_reset before switching");
  g.state_family = fam;
  return NAM_HIP_OK;
}

int refresh_map(nam_hip_batch* b, WidthGroup& g)
{
  if (g.d_map)
  {
    NAM_HIP_CHECK(quiesce(b));
    NAM_HIP_CHECK(g.d_map.reset());
  }
  bool identity = (int)g.streams.size() == b->n_streams;
  for (size_t i = 0; identity && i < g.streams.size(); i++)
    identity = g.streams[i] == (int)i;
  if (g.streams.empty() || identity)
    return NAM_HIP_OK;
  NAM_HIP_CHECK(upload(g.d_map, g.streams.data(), g.streams.size()));
  return NAM_HIP_OK;
}

// Which kernel a WaveNet group runs: explicit choice if possible, otherwise the fastest available.
constexpr size_t kKtAutoMaxStreams = 1024;

int pick_kernel(const nam_hip_batch* b, const WidthGroup& g)
{
  // a model bank runs its family's kernels for every launch shape (the other kernels know no banks): the interleaved-frame family,
  // what a one-model A2 batch runs under AUTO (select_kernel: nam_kq_kernel / nam_kt_mfma_kernel), or nam_wn_reg_kernel — at EVERY
  // stream count: the one-model rule below that hands a plain narrow model to nam_a1_kernel beyond kPersistTurns x per_cu x CUs
  // streams (another state layout) does not apply to a bank. An LSTM bank's group is no WaveNet group: select_kernel answers for
  // it (the gate-row kernels), nobody asks here. (api_bank.cpp: kBankFamily)
  if (g.d_bank_member && bank_rules(b).kernel_class != NAM_HIP_KERNEL_AUTO)
    return bank_rules(b).kernel_class;
  // ... and so does a container's batch at mixed sizes while it is one group on the bank path (SizeMix: mix_wanted has checked that
  // the class is one the batch's kernel choice admits)
  if (b->mix.resident && &g == &b->groups[(size_t)b->model->full_width])
    return mix_rules(b).kernel_class;
  const bool a1 = g.plan->a1.valid && g.d_a1;
  const bool mfma = a1 && (g.plan->a1.ws_ok || g.plan->a1.kt_ok);
  const bool il = a1 && g.plan->a1.il_ok && g.plan->a1.p2_ok; // the interleaved-frame kernels: the official topologies (compile-time job tables)
  const bool wr = g.plan->wr.ok && g.d_wr_blob;
  // a model no A1 kernel takes (FiLMs, gating, a nested condition_dsp ...) runs with its activations in registers when
  // its layers are among the instantiated shapes, else through the op interpreter
  const int fallback = a1 ? NAM_HIP_KERNEL_A1 : (wr ? NAM_HIP_KERNEL_WN_REG : NAM_HIP_KERNEL_GENERIC);
  switch (b->kernel)
  {
    case NAM_HIP_KERNEL_GENERIC: return NAM_HIP_KERNEL_GENERIC;
    case NAM_HIP_KERNEL_WN_REG: return wr ? NAM_HIP_KERNEL_WN_REG : fallback;
    case NAM_HIP_KERNEL_A1: return fallback;
    case NAM_HIP_KERNEL_A1_MFMA: return mfma ? NAM_HIP_KERNEL_A1_MFMA : fallback;
    case NAM_HIP_KERNEL_A1_IL: return il ? NAM_HIP_KERNEL_A1_IL : (mfma ? NAM_HIP_KERNEL_A1_MFMA : fallback);
    default: // AUTO
      // narrow models (1 .. 8 channels in the instantiated layer shapes) keep their whole dilation history in LDS on
      // nam_wn_reg_kernel; the VALU kernel fetches it from the HBM rings layer by layer
      if (!mfma)
      {
        // ... as long as the batch fits the chip that way (LDS image x streams per CU): beyond it no session can hold the
        // batch (its workgroups may take turns on the chip: kPersistTurns) and every buffer is a launch that moves the
        // image's windows in and out — a plain model then runs its HBM rings on the VALU kernel (A2-Lite, 105 KB of rings
        // per stream: 8.1 k xRT at any stream count with a launch per buffer, 13.2 k / 21.7 k / 40.5 k at 512 / 1,024 / 2,048
        // streams on the VALU kernel; 48.6 k in a session at 256).
        // Decided on the batch's stream count, which never changes: the two kernels keep different state layouts.
        if (wr && a1 && b->n_streams > wr_stream_bound(g.plan->wr.lds_bytes, b->n_cus)) // (a session's workgroups may take turns)
          return NAM_HIP_KERNEL_A1;
        return wr ? NAM_HIP_KERNEL_WN_REG : fallback;
      }
      // The K-tap kernel (A2 shapes) spreads a stream over four wavefronts: 2.3x the VALU kernel while the chip has
      // idle SIMDs, level with it at ~1,000 streams per GPU, behind it beyond (it issues more instructions per tap).
      if (!g.plan->a1.ws_ok && g.streams.size() > kKtAutoMaxStreams)
        return fallback;
      return NAM_HIP_KERNEL_A1_MFMA;
  }
}

// the session's side of a persistent launch of a one-wavefront-per-workgroup kernel (kernels.h: PersistArgs)
PersistArgs persist_args(const nam_hip_batch* b, const LaunchContext& ctx)
{
  PersistArgs pa;
  if (ctx.session_kind == PERSIST_NONE)
    return pa;
  pa.ring = b->ps.d_ring.get();
  pa.ring_mask = (int)kPRing - 1;
  pa.cons = b->ps.d_cons.get();
  pa.prog = b->ps.words.dev();
  pa.done = b->ps.words.dev() + b->ps.done_off;
  pa.seq0 = b->ps.seq0;
  pa.cmd0 = b->ps.cmd0;
  pa.grace = b->ps.grace;
  if (b->ps.cmd_done_published)
  {
    // the launch publishes every command (persist_launch decided), and lingers when the session does — beyond a microsecond,
    // as A1Args::p_linger counts (NAM_HIP_TICKET_LINGER_US = 0 or 1: the launch leaves as promptly as any other)
    const int ticks = session_lingers(b) ? session_linger_ticks(b) : 0;
    pa.linger = ticks > 100 ? ticks : 0;
    pa.cmd_count = b->ps.d_cmd_count.get();
    pa.cmd_done = b->ps.cmd_done.dev();
  }
  return pa;
}

// ... and of the workgroup-per-stream kernels (nam_a1_q_kernel, nam_a1_p4_kernel, nam_a1_p2_kernel, nam_kq_kernel), which carry the
// same words as A1Args::p_* plus where the results go and how long the launch lingers
static void session_args(const nam_hip_batch* b, const LaunchContext& ctx, A1Args& a)
{
  if (ctx.session_kind == PERSIST_NONE)
    return;
  const PersistArgs pa = persist_args(b, ctx);
  a.p_ring = pa.ring;
  a.p_ring_mask = pa.ring_mask;
  a.p_cons = pa.cons;
  a.p_prog = pa.prog;
  a.p_done = pa.done;
  a.p_seq0 = pa.seq0;
  a.p_cmd0 = pa.cmd0;
  a.p_grace = pa.grace;
  a.p_out_host = b->ps.out_is_host ? (b->ps.cmd_done_published ? 2 : 1) : 0;
  a.p_linger = session_lingers(b) ? session_linger_ticks(b) : 0;
  a.p_cmd_count = b->ps.d_cmd_count.get();
  a.p_cmd_done = b->ps.cmd_done.dev();
}

// What launch_policy.h: wr_launch_shape is asked about a launch of nam_wn_reg_kernel over these groups (launch_wr; persist_launch
// asks the same question ahead of a session's launch: wr_session_all_resident)
static WrShapeQuery wr_shape_query(const nam_hip_batch* b, WidthGroup* const* groups, const int* counts, int n_groups, int n_frames,
                                   const LaunchContext& ctx, int dense_forms)
{
  WrShapeQuery q;
  q.can_split = q.can_split4 = true;
  for (int k = 0; k < n_groups; k++)
  {
    const WrPlan& w = groups[k]->plan->wr;
    q.can_split = q.can_split && w.split_op[3] >= 1 && w.split_op[3] < (int)w.ops.size();
    q.can_split4 = q.can_split4 && w.split_op[0] >= 1 && w.split_op[0] < w.split_op[1] && w.split_op[1] < w.split_op[2]
                   && w.split_op[2] < (int)w.ops.size();
    q.total += counts[k];
    q.lds_bytes = std::max(q.lds_bytes, w.lds_bytes);
  }
  // (a session whose caller flushes after EVERY buffer is a series of one-buffer calls: nothing for a pipeline to overlap)
  const bool session = ctx.session_kind != PERSIST_NONE;
  const bool one_buffer_bursts = session && !b->pipe_session && b->ps.one_buffer_bursts();
  q.cus = b->n_cus;
  q.max_stages = b->wr_max_stages;
  q.dense_forms = dense_forms;
  q.multi_buffer = !b->no_pipe && !ctx.hints.one_buffer_call && !one_buffer_bursts && (session || n_frames > kBlock);
  return q;
}

// Will the session launch that launch_wr_all(b, gs, .., ctx) starts hold every workgroup on the chip at once, in the wavefront form
// it is started in (launch_policy.h: wr_all_resident)? The same query, the same answer: the host and the launch agree on lingering.
bool wr_session_all_resident(nam_hip_batch* b, const WrGroupList& gs, const LaunchContext& ctx)
{
  if (gs.n <= 0)
    return false;
  int counts[kWrMaxGroups];
  for (int k = 0; k < gs.n; k++)
    counts[k] = (int)gs.g[k]->streams.size();
  const std::string& module = gs.g[0]->plan->wr.jit_module;
  const WrJitFunctions jit = module.empty() ? WrJitFunctions() : wr_jit_functions(module, b->device);
  if (jit.rc != NAM_HIP_OK)
    return false; // (the launch itself reports it)
  const WrShapeQuery q = wr_shape_query(b, gs.g, counts, gs.n, kBlock, ctx, jit.dense_forms());
  return wr_all_resident(q, wr_launch_shape(q));
}

// nam_wn_reg_kernel over up to kWrMaxGroups width groups in ONE launch (kernels.h: WrArgs): group k's `counts[k]` streams
// (`maps[k]`: position -> stream index, nullptr = identity) become consecutive workgroups.
int launch_wr(nam_hip_batch* b, WidthGroup* const* groups, const int* const* maps, const int* counts, int n_groups,
              const float* d_in, float* d_out, int n_frames, long io_stride, hipStream_t s, const LaunchContext& ctx)
{
  // 1. the arguments, from the groups
  WrArgs a;
  std::memset(&a, 0, sizeof(a));
  int total = 0;
  bool layers = false, runs = false, rt_layers = false;
  for (int k = 0; k < n_groups; k++)
  {
    WidthGroup& g = *groups[k];
    const WrPlan& w = g.plan->wr;
    layers = layers || w.has_layers;
    runs = runs || w.has_runs;
    rt_layers = rt_layers || w.has_rt_layers;
    if (const int rc = claim_state_family(g, STATE_WN_REG))
      return rc;
    WrGroup& G = a.g[k];
    G.blob = g.d_wr_blob.get();
    G.state = g.d_state.get();
    G.stream_map = maps[k];
    G.state_stride = g.state_stride;
    G.n_ops = (int)w.ops.size();
    G.blob_floats = (int)w.blob.size();
    G.hist_floats = w.hist_floats;
    G.n_slots = w.n_layers;
    G.tab_rows = w.tab_rows;
    G.n_rows = w.n_rows;
    G.tab_pf = w.tab_pf;
    G.n_pf = w.n_pf;
    G.tab_ring = w.tab_ring;
    G.tab_ops = w.tab_ops;
    G.first = total;
    for (int q = 0; q < 3; q++)
      G.split_op[q] = w.split_op[q];
    G.prog = w.program;
    total += counts[k];
  }
  a.n_groups = n_groups;
  a.in = d_in;
  a.out = d_out;
  a.io_stride = io_stride;
  a.n_frames = n_frames;
  a.in_ch = groups[0]->plan->in_channels;
  a.out_ch = groups[0]->plan->out_channels;
  a.ps = persist_args(b, ctx);
  a.bank_member = groups[0]->d_bank_member.get(); // (a bank batch has one group: groups[0]->d_wr_blob is [members][bank_stride])
  a.bank_stride = groups[0]->bank_stride;
  // every group on the model's own code object (they share one: build_model), or every group on the ahead-of-time kernel
  const std::string& module = groups[0]->plan->wr.jit_module;
  for (int k = 1; k < n_groups; k++)
    if (groups[k]->plan->wr.jit_module != module)
      return fail(NAM_HIP_ERR_INVALID_ARGUMENT, "nam_wn_reg_kernel: the groups of one launch run different code objects");
  const WrJitFunctions jit = module.empty() ? WrJitFunctions() : wr_jit_functions(module, b->device);
  if (jit.rc != NAM_HIP_OK)
    return jit.rc;
  // 2. how many wavefronts per stream, and which build of them (launch_policy.h): more than one only when the launch holds more
  // than one buffer
  const WrShapeQuery q = wr_shape_query(b, groups, counts, n_groups, n_frames, ctx, jit.dense_forms());
  const WrLaunchShape shape = wr_launch_shape(q);
  const int stages = shape.stages;
  if (q.multi_buffer)
  {
    if (stats_on() && (stages != b->wr_last_stages || shape.dense != b->wr_last_dense))
      std::fprintf(stderr, "nam_hip nam_wn_reg_kernel: %d workgroups as %d wavefront(s) per stream%s, %d bytes of LDS each\n", total, stages,
                   shape.dense ? " (two per SIMD)" : "", shape.lds_bytes);
    b->wr_last_stages = stages;
    b->wr_last_dense = shape.dense;
  }
  // 3. the launch, as `stages` wavefronts per stream
  const int lds_bytes = shape.lds_bytes;
  if (stages == 2) // (the kernels read a two-wave launch's cut from [1]: WrGroup::split_op)
    for (int k = 0; k < n_groups; k++)
      a.g[k].split_op[1] = groups[k]->plan->wr.split_op[3];
  if (!module.empty())
  {
    void* const fn = jit.pick(stages, shape.dense);
    NAM_HIP_CHECK(launch_wn_reg_jit(fn, a, total, lds_bytes, stages, LaunchStream(s, ctx.retired)));
    return NAM_HIP_OK;
  }
  NAM_HIP_CHECK(launch_wn_reg(a, total, lds_bytes, layers, runs, rt_layers, stages, LaunchStream(s, ctx.retired)));
  return NAM_HIP_OK;
}

WrGroupList wr_groups(nam_hip_batch* b)
{
  WrGroupList out;
  const Plan& full = *b->groups[b->model->full_width].plan;
  for (auto& g : b->groups)
  {
    if (g.streams.empty())
      continue;
    if (out.n == kWrMaxGroups || g.plan->arch != ARCH_WAVENET || !g.d_wr_blob || pick_kernel(b, g) != NAM_HIP_KERNEL_WN_REG
        || g.plan->in_channels != full.in_channels || g.plan->out_channels != full.out_channels
        || (out.n > 0 && g.plan->wr.jit_module != out.g[0]->plan->wr.jit_module)) // (one launch = one code object)
    {
      out.n = 0;
      return out;
    }
    out.g[out.n++] = &g;
  }
  return out;
}
int launch_wr_all(nam_hip_batch* b, const WrGroupList& gs, const float* d_in, float* d_out, int n_frames, long io_stride,
                  hipStream_t s, const LaunchContext& ctx)
{
  const int* maps[kWrMaxGroups];
  int counts[kWrMaxGroups];
  for (int k = 0; k < gs.n; k++)
  {
    maps[k] = gs.g[k]->d_map.get();
    counts[k] = (int)gs.g[k]->streams.size();
  }
  return launch_wr(b, gs.g, maps, counts, gs.n, d_in, d_out, n_frames, io_stride, s, ctx);
}

// The WaveNet kernel a launch of n_frames runs: pick_kernel, except that under AUTO a launch that walks several blocks
// (offline render, prewarm) takes the interleaved-frame kernel — the faster one inside a launch (9.3 vs 11.2 us per
// block at 256 streams; its longer prologue only hurts one-block launches). Same rings, same write positions: the two
// alternate freely.
int kernel_for_launch(const nam_hip_batch* b, const WidthGroup& g, int n_frames)
{
  const int kernel = pick_kernel(b, g);
  if (b->kernel == NAM_HIP_KERNEL_AUTO && kernel == NAM_HIP_KERNEL_A1_MFMA && g.plan->a1.ws_ok && g.plan->a1.il_ok && g.plan->a1.p2_ok
      && n_frames >= 4 * kBlock)
    return NAM_HIP_KERNEL_A1_IL;
  return kernel;
}

// ... and of a launch in general: the resident launch of a session of the interleaved-frame family runs that family whatever a
// one-buffer launch of the batch would (persist_kind: PERSIST_A1_P2 needs no more than AUTO and a model the family takes)
static int family_for_launch(const nam_hip_batch* b, const WidthGroup& g, int n_frames, const LaunchContext& ctx)
{
  return ctx.session_kind == PERSIST_A1_P2 ? NAM_HIP_KERNEL_A1_IL : kernel_for_launch(b, g, n_frames);
}

// the functions as rocprofv3 --kernel-trace shows them, without template arguments (in KernelFn's order)
static const char* const kKernelFnName[KERNEL_FN_COUNT] = {
  "nam_generic_kernel", "nam_wn_reg_kernel", "nam_a1_kernel", "nam_a1_mfma_kernel", "nam_kt_mfma_kernel", "nam_kq_kernel",
  "nam_a1_p2_kernel", "nam_a1_p4_kernel", "nam_a1_q_kernel", // WaveNets
  "nam_lstm_kernel", "nam_lstm_mfma_kernel", "nam_lstm_mfma_reg_kernel", "nam_lstm_row_kernel", "nam_lstm_wide_kernel",
  "nam_linear_kernel"};

// Which __global__ function the group runs for a launch of `n_frames` in the context `ctx`: what launch_group launches and what
// nam_hip_batch_kernel_name reports.
static KernelFn select_kernel(const nam_hip_batch* b, const WidthGroup& g, int n_frames, const LaunchContext& ctx)
{
  const Plan& p = *g.plan;
  const bool session = ctx.session_kind != PERSIST_NONE;
  if (p.arch == ARCH_LINEAR) // one device engine for every Linear model, launch length and stream count
    return FN_LINEAR;
  if (p.arch != ARCH_WAVENET) // (ARCH_LSTM: a container's groups carry their submodels' plans)
  {
    // AUTO: small cells (hidden <= 4) one gate row per lane and four streams per wavefront, cells of 5 .. 32 units two
    // gate rows per lane and one stream per wavefront, else the matrix-core kernel (16 streams per wavefront);
    // NAM_HIP_KERNEL_A1_MFMA forces the matrix-core kernel; NAM_HIP_KERNEL_GENERIC: lanes = streams
    // A model bank runs the first two whatever b->kernel says (kBankFamily: the LSTM family's functions): the other LSTM kernels
    // share one wavefront's weights among their streams and know no banks (api_bank.cpp admits only cells one of the two takes)
    const bool small = g.d_bank_member || (b->kernel != NAM_HIP_KERNEL_GENERIC && b->kernel != NAM_HIP_KERNEL_A1_MFMA);
    if (small && lstm_row_eligible(p.lstm))
      return FN_LSTM_ROW;
    if (small && lstm_wide_eligible(p.lstm))
      return FN_LSTM_WIDE;
    if (p.lstm.mf_ok && b->kernel != NAM_HIP_KERNEL_GENERIC)
      return lstm_mfma_in_registers(p.lstm) ? FN_LSTM_MFMA_REG : FN_LSTM_MFMA;
    return FN_LSTM;
  }
  if (ctx.session_kind == PERSIST_WN_REG) // (one launch for every width group: launch_wr_all)
    return FN_WN_REG;
  // nam_a1_p4_kernel / nam_a1_q_kernel / nam_kq_kernel (pipelines, consecutive buffers in flight at once) instead of the
  // one-buffer kernels: whenever a launch holds more than one buffer — a persistent session, an offline render, a prewarm. A
  // launch of one block has nothing to overlap (every stage waits for the one before).
  const bool pipeline = !b->no_pipe && (session || n_frames > kBlock);
  switch (family_for_launch(b, g, n_frames, ctx))
  {
    case NAM_HIP_KERNEL_GENERIC: return FN_GENERIC;
    case NAM_HIP_KERNEL_WN_REG: return FN_WN_REG;
    case NAM_HIP_KERNEL_A1: return FN_A1;
    case NAM_HIP_KERNEL_A1_IL:
      if (!pipeline) // one buffer: the four-wave kernel, job table compiled in
        return FN_A1_P2;
      // the 16 / 8 topology as twelve one-wave stages, most rings resident in LDS (kernel_a1_q.hip) — unless the caller waits for
      // the FIRST buffer (CallHints::short_blocking_call; PersistSession::short_bursts, which ticket sessions never follow) —
      // else as a pipeline of wave sets (three wavefronts per SIMD) across consecutive buffers
      if (q_runs(b, p) && !ctx.hints.short_blocking_call && !(session && !b->pipe_session && b->ps.short_bursts()))
        return FN_A1_Q;
      return FN_A1_P4;
    default: // NAM_HIP_KERNEL_A1_MFMA
      if (p.a1.ws_ok)
        return FN_A1_MFMA;
      // the K-tap kernel addresses the launch's input through a 32-bit buffer descriptor (1 GiB of float32 audio per
      // stream and launch): longer launches take the VALU kernel, same state layout
      if (n_frames > (1 << 28))
        return FN_A1;
      // the A2 topology with more than one buffer in the launch (a session, a render, a prewarm): the pipeline of one-wave
      // stages compiled for it (kernel_kq.hip); same state as the K-tap kernel
      if (kq_runs(b, p) && pipeline)
        return FN_KQ;
      return FN_KT_MFMA; // single-array models with other kernel sizes than 3 (A2): the K-tap MFMA kernel
  }
}

// Name of the __global__ function launch_group runs for this group (what rocprofv3 --kernel-trace reports, without
// template arguments): lets callers attribute measurements to the right kernel.
// `n_frames`: the launch length the question is about (under AUTO a launch of four or more blocks runs another kernel
// of the family than a one-block launch); 64 in persistent mode means "a command of the session" — answered for what the
// NEXT launch of the session starts (PersistSession::short_bursts: the burst history outlives a session), outside any host call
const char* group_kernel_name(const nam_hip_batch* b, const WidthGroup& g, int n_frames)
{
  const bool session_command = b->ps.enabled && n_frames == kBlock;
  return kKernelFnName[select_kernel(b, g, n_frames, LaunchContext{session_command ? persist_kind(b) : (int)PERSIST_NONE})]; // (no hints)
}

// what every kernel's argument block starts with (kernels.h): the group's weights and state, the launch's streams and audio
template <typename Args>
static void common_args(Args& a, const WidthGroup& g, const int* d_map, const float* d_in, float* d_out, int n_frames, long io_stride)
{
  a.blob = g.d_blob.get();
  a.state = g.d_state.get();
  a.state_stride = g.state_stride;
  a.stream_map = d_map;
  a.in = d_in;
  a.out = d_out;
  a.io_stride = io_stride;
  a.n_frames = n_frames;
}

// the arrays' activation when it is uniform (a compile-time specialised kernel), else -1 (run-time dispatch)
static int uniform_act(const A1Plan& a1)
{
  for (int i = 1; i < a1.n_arrays; i++)
    if (a1.arr[i].act != a1.arr[0].act)
      return -1;
  return a1.arr[0].act;
}

// first float of a submodel's blob a mixed-size residency's device image keeps (mix_prepare cuts there, the launch rebases on it)
static int mix_blob_base(const Plan& p, const MixFamilyRules& r)
{
  return r.blob_source == BANK_BLOB_KERNEL_REGION ? p.a1.ws_tiles_off : 0;
}

static int launch_a1_family(nam_hip_batch* b, WidthGroup& g, KernelFn fn, A1Args& a, int n, hipStream_t stream, const LaunchContext& ctx)
{
  const LaunchStream s(stream, ctx.retired); // (for the session-capable kernels; the others take the bare stream)
  const Plan& p = *g.plan;
  a.plan = g.d_a1.get();
  a.act_p0 = p.a1.arr[0].act_p0; // uniform across arrays and layers for the A1 kernels (plan.cpp)
  a.dbg = ctx.dbg;
  if (ctx.session_kind != PERSIST_NONE && b->ps.why)
    a.dbg = b->ps.why.dev(); // (NAM_HIP_SESSION_STATS: why a lingering workgroup left — il_common.h: session_wait_command)
  a.n_rings = p.a1.n_rings;
  a.head_scale = p.blob[(size_t)p.a1.head_scale_off];
  a.bank_member = g.d_bank_member.get();
  a.bank_scal = g.d_bank_scal.get();
  a.bank_stride = g.bank_stride;
  const bool il = fn == FN_A1_P2 || fn == FN_A1_P4 || fn == FN_A1_Q;
  if (g.d_bank_member && !((bank_rules(b).fns >> fn) & 1u))
    return fail(NAM_HIP_ERR_UNSUPPORTED, bank_rules(b).launch_refusal);
  if (b->mix.resident)
  {
    // a container at mixed sizes (SizeMix): every stream's rings are in this group's rows, its weights are its submodel's (padded)
    // blob — the bank path of the family's kernels, which are the ones that know it
    if (&g != &b->groups[(size_t)b->model->full_width] || !((mix_rules(b).fns >> fn) & 1u))
      return fail(NAM_HIP_ERR_UNSUPPORTED, mix_rules(b).launch_refusal);
    a.blob = b->mix.d_blob.get();
    a.bank_member = b->mix.d_member.get();
    a.bank_scal = b->mix.d_scal.get();
    a.bank_stride = b->mix.stride;
  }
  if (il)
  {
    const int act = uniform_act(p.a1);
    // a bank's rows start at the kernels' region of the blob (api_bank.cpp): offsets from there
    const int base = g.d_bank_member ? bank_blob_base(p, b->bank->family) : b->mix.resident ? mix_blob_base(p, mix_rules(b)) : 0;
    a.tiles_off = p.a1.ws_tiles_off - base;
    a.consts_off = p.a1.ws_consts_off - base;
    a.xt_off = p.a1.ws_xt_off - base;
    a.n_xt = p.a1.ws_n_xt;
    a.act = act;
    session_args(b, ctx, a);
    if (!p.a1.p2_ok) // (pick_kernel: the interleaved-frame kernels exist for the official topologies' compile-time tables only)
      return fail(NAM_HIP_ERR_UNSUPPORTED, "NAM_HIP_KERNEL_A1_IL: not one of the official topologies");
    if (fn == FN_A1_Q)
    {
      // its own weight block + the FULL-layout tiles of array 0 (kept in registers)
      a.consts_off = p.a1.ws_tiles_off - base;
      a.tiles_off = p.a1.q_w_off - base;
      NAM_HIP_CHECK(launch_a1_q(a, n, act, s));
    }
    else if (fn == FN_A1_P4)
      NAM_HIP_CHECK(launch_a1_p4(a, n, p.a1.p2_c0, p.a1.p2_c1, act, s));
    else
      NAM_HIP_CHECK(launch_a1_p2(a, n, p.a1.p2_c0, p.a1.p2_c1, act, s));
  }
  else if (fn == FN_KQ)
  {
    a.tiles_off = p.a1.kq_w_off;
    a.consts_off = p.a1.kt_lds_src_off;
    a.r1_off = p.a1.kt_rech_off;
    a.act = p.a1.arr[0].act;
    session_args(b, ctx, a);
    NAM_HIP_CHECK(launch_kq(a, n, p.a1.arr[0].act, s));
  }
  else if (fn == FN_KT_MFMA)
    NAM_HIP_CHECK(launch_kt_mfma(a, n, p.a1.kt_nk, p.a1.arr[0].channels, p.a1.kt_lds_floats, p.a1.arr[0].act, stream));
  else if (fn == FN_A1_MFMA)
  {
    a.n_mjobs = p.a1.ws_jobs;
    a.tiles_off = p.a1.ws_tiles_off;
    a.consts_off = p.a1.ws_consts_off;
    a.r1_off = p.a1.ws_r1_off;
    a.xt_off = p.a1.ws_xt_off;
    a.n_xt = p.a1.ws_n_xt;
    a.lds_tiles_b = p.a1.ws_lds_tiles_b;
    a.lds_xt_b = p.a1.ws_lds_xt_b;
    a.lds_cond_b = p.a1.ws_lds_cond_b;
    a.lds_bytes = p.a1.ws_lds_bytes;
    a.prefetch = p.a1.ws_prefetch;
    NAM_HIP_CHECK(launch_a1_mfma(a, n, uniform_act(p.a1), stream));
  }
  else
    NAM_HIP_CHECK(launch_a1(a, n, stream));
  return NAM_HIP_OK;
}

static int launch_generic_program(const WidthGroup& g, GenericArgs& a, int n, hipStream_t s)
{
  const Plan& p = *g.plan;
  a.ops = g.d_ops.get();
  a.in_ch = p.in_channels;
  a.out_ch = p.out_channels;
  // conv weights from LDS when the model's weights fit next to the activation rows (kernels.h)
  int lds_bytes = p.lds_rows * kBlock * (int)sizeof(float);
  a.w_lds_off = p.lds_rows * kBlock;
  a.blob_floats = 0;
  if (lds_bytes + p.generic_blob_floats * (int)sizeof(float) <= 96 * 1024)
  {
    a.blob_floats = p.generic_blob_floats;
    lds_bytes += p.generic_blob_floats * (int)sizeof(float);
  }
  NAM_HIP_CHECK(launch_generic(a, n, lds_bytes, s));
  return NAM_HIP_OK;
}

static int launch_lstm_family(nam_hip_batch* b, WidthGroup& g, KernelFn fn, LSTMArgs& a, int n, hipStream_t s, const LaunchContext& ctx)
{
  a.n_streams = n;
  if (fn == FN_LSTM_ROW || fn == FN_LSTM_WIDE)
  {
    a.bank_member = g.d_bank_member.get(); // (a bank: a.blob is [members][bank_stride], whole plan blobs)
    a.bank_stride = g.bank_stride;
    a.ps = persist_args(b, ctx);
    NAM_HIP_CHECK(fn == FN_LSTM_ROW ? launch_lstm_row(a, {s, ctx.retired}) : launch_lstm_wide(a, {s, ctx.retired}));
  }
  else if (fn == FN_LSTM_MFMA || fn == FN_LSTM_MFMA_REG) // (launch_lstm_mfma tells the two apart: lstm_mfma_in_registers)
    NAM_HIP_CHECK(launch_lstm_mfma(a, s));
  else
  {
    // a cell whose columns exceed a CU's LDS keeps them in global memory (the reference has no size limit,
    // lstm.cpp:31-68): slower, but it runs
    const long need = lstm_scratch_floats(a);
    if (need > g.scratch_floats)
    {
      NAM_HIP_CHECK(hipStreamSynchronize(s));
      g.scratch_floats = 0;
      NAM_HIP_CHECK(g.d_scratch.reset());
      NAM_HIP_CHECK(hipMalloc(g.d_scratch.out(), (size_t)need * sizeof(float)));
      g.scratch_floats = need;
    }
    a.scratch = g.d_scratch.get();
    NAM_HIP_CHECK(launch_lstm(a, s));
  }
  return NAM_HIP_OK;
}

// A Linear batch's launch: cut into pieces of at most the batch's piece length (plan.h: LinearPlan::piece_frames), each piece
// append + compute + reduce behind one another on `s` (kernel_linear.hip). The ring position is host state, advanced per piece.
static int launch_linear_group(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n, const float* d_in, float* d_out, int n_frames,
                               long io_stride, hipStream_t s)
{
  const LinearPlan& L = g.plan->linear;
  if (d_map || n != b->n_streams || !g.d_lin_hist)
    return fail(NAM_HIP_ERR_INVALID_ARGUMENT, "Linear: a launch covers every stream of the batch (one shared history ring)");
  LinearArgs a;
  a.blob = g.d_blob.get();
  a.hist = g.d_lin_hist.get();
  a.part = g.d_lin_part.get();
  a.io_stride = io_stride;
  a.n_streams = n;
  a.in_ch = L.in_ch;
  a.out_ch = L.out_ch;
  a.cols_per_stream = L.cols_per_stream;
  a.n_cols = n * L.cols_per_stream;
  a.cols_pad = g.lin_cols_pad;
  a.hist_frames = g.lin_hist_frames;
  a.part_frames = g.lin_part_frames;
  a.n_splits = L.n_splits;
  a.split_taps = L.split_taps;
  a.taps_off = L.taps_off;
  a.bias = L.bias;
  for (int at = 0; at < n_frames; at += g.lin_piece)
  {
    a.n_frames = std::min(g.lin_piece, n_frames - at);
    a.in = d_in ? d_in + at : nullptr;
    a.out = d_out ? d_out + at : nullptr;
    a.pos = g.lin_pos;
    NAM_HIP_CHECK(launch_linear(a, s));
    g.lin_pos = (g.lin_pos + a.n_frames) % g.lin_hist_frames;
  }
  return NAM_HIP_OK;
}

// ---- an all-Linear container's batch (api_internal.h: LinearContainer) ----

bool lin_container_model(const nam_hip_model& m)
{
  return m.spec->arch == ARCH_CONTAINER && !m.plans.empty() && m.plans[0].arch == ARCH_LINEAR; // (the loader admits all or none)
}

int lin_container_hist_frames(const nam_hip_model& m, int max_frames)
{
  int taps = 0;
  for (const Plan& p : m.plans)
    taps = std::max(taps, p.linear.n_splits * p.linear.split_taps);
  return taps + m.plans[0].linear.piece_frames(max_frames); // (the piece depends on max_frames alone)
}

// The work list of the streams' current assignment (b->stream_width), checked against what creation allocated, to the device.
// Control calls only: allocates host memory and copies synchronously.
static int lin_container_upload(nam_hip_batch* b)
{
  LinearContainer& lc = b->lin;
  if (!build_linear_worklist(b->stream_width.data(), b->n_streams, lc.subs.data(), (int)lc.subs.size(), lc.work)
      || (int64_t)lc.work.pairs.size() > lc.caps.max_pairs || lc.work.part_slabs > lc.caps.max_part_slabs || lc.work.grid_splits > lc.caps.max_splits
      || (int)lc.work.col_pair.size() != lc.caps.cols_pad)
    return fail(NAM_HIP_ERR_MODEL, "Linear container: the work list exceeds what the batch allocated");
  NAM_HIP_CHECK(hipMemcpy(lc.d_pairs.get(), lc.work.pairs.data(), lc.work.pairs.size() * sizeof(LinearPair), hipMemcpyHostToDevice));
  NAM_HIP_CHECK(hipMemcpy(lc.d_col_pair.get(), lc.work.col_pair.data(), lc.work.col_pair.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return NAM_HIP_OK;
}

int lin_container_create(nam_hip_batch* b)
{
  const nam_hip_model& m = *b->model;
  LinearContainer& lc = b->lin;
  if (b->n_streams > (1 << 24))
    return fail(NAM_HIP_ERR_UNSUPPORTED, "Linear: more than 16,777,216 columns (streams x channels) in one batch");
  std::vector<float> blob;
  for (const Plan& p : m.plans)
  {
    LinearSub s;
    s.n_splits = p.linear.n_splits;
    s.split_taps = p.linear.split_taps;
    s.taps_off = (int32_t)blob.size() + p.linear.taps_off;
    s.bias = p.linear.bias;
    lc.subs.push_back(s);
    blob.insert(blob.end(), p.blob.begin(), p.blob.end());
  }
  lc.caps = linear_work_caps(b->n_streams, lc.subs.data(), (int)lc.subs.size());
  if (lc.caps.max_part_slabs > INT32_MAX)
    return fail(NAM_HIP_ERR_UNSUPPORTED, "Linear container: too many streams x K-splits for one batch");
  lc.piece = m.plans[0].linear.piece_frames(b->max_frames);
  lc.part_frames = (lc.piece + kBlock - 1) / kBlock * kBlock;
  lc.hist_frames = lin_container_hist_frames(m, b->max_frames);
  lc.pos = 0;
  NAM_HIP_CHECK(upload(lc.d_blob, blob.data(), blob.size()));
  const size_t hist_bytes = (size_t)lc.hist_frames * lc.caps.cols_pad * sizeof(float);
  NAM_HIP_CHECK(hipMalloc(lc.d_hist.out(), hist_bytes));
  NAM_HIP_CHECK(hipMalloc(lc.d_part.out(), (size_t)linear_part_floats(lc.caps.max_part_slabs, lc.part_frames) * sizeof(float)));
  NAM_HIP_CHECK(hipMalloc(lc.d_pairs.out(), (size_t)lc.caps.max_pairs * sizeof(LinearPair)));
  NAM_HIP_CHECK(hipMalloc(lc.d_col_pair.out(), (size_t)lc.caps.cols_pad * sizeof(int32_t)));
  NAM_HIP_CHECK(hipMemsetAsync(lc.d_hist.get(), 0, hist_bytes, b->stream.get())); // history starts at zero (Buffer, dsp.cpp:203-230)
  lc.on = true;
  return lin_container_upload(b);
}

// As launch_linear_group: pieces of at most lc.piece frames, each append + pairs + reduce on `s`; the ring position advances per piece.
int lin_container_launch(nam_hip_batch* b, const float* d_in, float* d_out, int n_frames, long io_stride, hipStream_t s)
{
  LinearContainer& lc = b->lin;
  LinearPairsArgs p;
  LinearArgs& a = p.a;
  a.blob = lc.d_blob.get();
  a.hist = lc.d_hist.get();
  a.part = lc.d_part.get();
  a.io_stride = io_stride;
  a.n_streams = a.n_cols = b->n_streams;
  a.in_ch = a.out_ch = a.cols_per_stream = 1;
  a.cols_pad = lc.caps.cols_pad;
  a.hist_frames = lc.hist_frames;
  a.part_frames = lc.part_frames;
  a.n_splits = lc.work.grid_splits;
  a.split_taps = lc.caps.max_split_taps;
  a.taps_off = 0;
  a.bias = 0.0f;
  p.pairs = lc.d_pairs.get();
  p.col_pair = lc.d_col_pair.get();
  p.n_pairs = (int)lc.work.pairs.size();
  p.hist_taps = lc.caps.max_hist_taps;
  for (int at = 0; at < n_frames; at += lc.piece)
  {
    a.n_frames = std::min(lc.piece, n_frames - at);
    a.in = d_in ? d_in + at : nullptr;
    a.out = d_out ? d_out + at : nullptr;
    a.pos = lc.pos;
    NAM_HIP_CHECK(launch_linear_pairs(p, s));
    lc.pos = (lc.pos + a.n_frames) % lc.hist_frames;
  }
  return NAM_HIP_OK;
}

int lin_container_move(nam_hip_batch* b, const std::vector<int>& moved, int w, bool zero_columns)
{
  LinearContainer& lc = b->lin;
  for (int s : moved)
  {
    auto& old = b->groups[(size_t)b->stream_width[(size_t)s]].streams;
    old.erase(std::remove(old.begin(), old.end(), s), old.end());
    b->stream_width[(size_t)s] = w;
    b->groups[(size_t)w].streams.push_back(s);
  }
  std::sort(b->groups[(size_t)w].streams.begin(), b->groups[(size_t)w].streams.end());
  // a freshly reset submodel (container.cpp:85-97 + Reset): the stream's column is zero over the whole ring; the position and every
  // other column stay
  for (size_t i = 0; zero_columns && i < moved.size(); i++)
    NAM_HIP_CHECK(launch_linear_stream_cols(lc.d_hist.get(), lc.hist_frames, lc.caps.cols_pad, lc.pos, moved[i], 1, nullptr, LINEAR_COLS_ZERO,
                                            b->stream.get()));
  NAM_HIP_CHECK(hipStreamSynchronize(b->stream.get()));
  return lin_container_upload(b);
}

// Launch one group's kernel over `n` streams given by `d_map` (nullptr = streams 0..n-1).
int launch_group(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n, const float* d_in, float* d_out,
                 int n_frames, long io_stride, hipStream_t s, const LaunchContext& ctx)
{
  if (n <= 0 || n_frames <= 0)
    return NAM_HIP_OK;
  const Plan& p = *g.plan;
  const KernelFn fn = select_kernel(b, g, n_frames, ctx);
  if (fn == FN_LINEAR)
    return launch_linear_group(b, g, d_map, n, d_in, d_out, n_frames, io_stride, s);
  if (p.arch != ARCH_WAVENET)
  {
    LSTMArgs a = lstm_args(p.lstm);
    common_args(a, g, d_map, d_in, d_out, n_frames, io_stride);
    return launch_lstm_family(b, g, fn, a, n, s, ctx);
  }
  if (const int rc = claim_state_family(g, state_family_of(p, family_for_launch(b, g, n_frames, ctx))))
    return rc;
  if (fn == FN_WN_REG)
  {
    WidthGroup* one[1] = {&g};
    const int* maps[1] = {d_map};
    const int counts[1] = {n};
    return launch_wr(b, one, maps, counts, 1, d_in, d_out, n_frames, io_stride, s, ctx);
  }
  if (fn == FN_GENERIC)
  {
    GenericArgs a;
    common_args(a, g, d_map, d_in, d_out, n_frames, io_stride);
    return launch_generic_program(g, a, n, s);
  }
  A1Args a;
  common_args(a, g, d_map, d_in, d_out, n_frames, io_stride);
  return launch_a1_family(b, g, fn, a, n, s, ctx);
}

// DSP::prewarm (NAM/dsp.cpp:67-101): process whole max_frames-sized buffers of silence until at
// least prewarm_samples have gone through.
int prewarm_frames(const nam_hip_batch* b, const Plan& p)
{
  const int bs = std::max(b->max_frames, 1);
  if (p.prewarm_samples <= 0)
    return 0;
  return (p.prewarm_samples + bs - 1) / bs * bs;
}

// `first_stream`: one of the n streams (its state seeds the prewarm cache).
int reset_streams(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n, bool prewarm, int first_stream)
{
  if (n <= 0)
    return NAM_HIP_OK;
  const Plan& p = *g.plan;
  if (p.arch == ARCH_LINEAR)
  {
    // the history of a freshly constructed reference model: zeros (include/nam_hip.h: the reference's two engines keep different
    // things across Reset). No prewarm: GetPrewarmSamples() is 0 (dsp.h:153)
    NAM_HIP_CHECK(hipMemsetAsync(g.d_lin_hist.get(), 0, (size_t)g.lin_hist_frames * g.lin_cols_pad * sizeof(float), b->stream.get()));
    g.lin_pos = 0;
    return NAM_HIP_OK;
  }
  const int frames = prewarm ? prewarm_frames(b, p) : 0;
  const bool all = n == (int)g.streams.size();
  if (p.arch == ARCH_WAVENET)
  {
    if (frames > 0 && g.d_prewarm)
    {
      // a state cached by the same kernel over the same number of frames: copy it (every stream's is identical)
      const int kernel = kernel_for_launch(b, g, frames);
      const StateFamily fam = state_family_of(p, kernel);
      if (g.prewarm_kernel == kernel && g.prewarm_len == frames && (all || g.state_family == STATE_FRESH || g.state_family == fam))
      {
        NAM_HIP_CHECK(launch_fill_state(g.d_state.get(), g.state_stride, d_map, n, g.d_prewarm.get(), p.state_floats, p.state_floats, b->stream.get()));
        g.state_family = fam;
        return NAM_HIP_OK;
      }
    }
    NAM_HIP_CHECK(launch_fill_state(g.d_state.get(), g.state_stride, d_map, n, nullptr, 0, p.state_floats, b->stream.get()));
    if (all)
      g.state_family = STATE_FRESH; // every stream of the group is zeroed: either layout may follow
  }
  if (frames > 0)
  {
    const int rc = launch_group(b, g, d_map, n, nullptr, nullptr, frames, 0, b->stream.get(), LaunchContext());
    if (rc != NAM_HIP_OK)
      return rc;
    if (p.arch == ARCH_WAVENET && first_stream >= 0 && !g.d_bank_member) // (a bank's prewarmed state depends on the member: no cache)
    {
      if (!g.d_prewarm)
        NAM_HIP_CHECK(hipMalloc(g.d_prewarm.out(), (size_t)p.state_floats * sizeof(float)));
      NAM_HIP_CHECK(hipMemcpyAsync(g.d_prewarm.get(), g.d_state.get() + (size_t)first_stream * g.state_stride,
                                   (size_t)p.state_floats * sizeof(float), hipMemcpyDeviceToDevice, b->stream.get()));
      g.prewarm_kernel = kernel_for_launch(b, g, frames);
      g.prewarm_len = frames;
    }
  }
  return NAM_HIP_OK;
}

// The tail of nam_hip_batch_set_slimmable_size and bank_set_stream_model (api_internal.h)
// (`moved.front()` seeds the prewarm cache; a bank group has none: reset_streams)
int reset_moved_streams(nam_hip_batch* b, WidthGroup& g, const std::vector<int>& moved, bool fill_initial_states)
{
  DeviceBuf<int> d_moved;
  NAM_HIP_CHECK(upload(d_moved, moved.data(), moved.size()));
  int rc = fill_initial_states ? bank_fill_initial_state(b, g, d_moved.get(), (int)moved.size()) : NAM_HIP_OK;
  if (rc == NAM_HIP_OK)
    rc = reset_streams(b, g, d_moved.get(), (int)moved.size(), b->was_reset && b->reset_with_prewarm, moved.front());
  const hipError_t e = hipStreamSynchronize(b->stream.get()); // (before d_moved goes: the launches read it)
  if (rc != NAM_HIP_OK)
    return rc;
  NAM_HIP_CHECK(e);
  return NAM_HIP_OK;
}

int collect_stream_ids(const nam_hip_batch* b, const int* stream_ids, int n_ids, const char* who, std::vector<int>& ids)
{
  ids.clear();
  if (!stream_ids)
  {
    ids.resize((size_t)b->n_streams);
    for (int i = 0; i < b->n_streams; i++)
      ids[(size_t)i] = i;
    return NAM_HIP_OK;
  }
  for (int i = 0; i < n_ids; i++)
  {
    if (stream_ids[i] < 0 || stream_ids[i] >= b->n_streams)
      return fail(NAM_HIP_ERR_INVALID_ARGUMENT, std::string(who) + ": stream id out of range");
    ids.push_back(stream_ids[i]);
  }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  return NAM_HIP_OK;
}

int move_streams_to_width(nam_hip_batch* b, const std::vector<int>& moved, int w)
{
  for (int s : moved)
  {
    auto& old = b->groups[(size_t)b->stream_width[(size_t)s]].streams;
    old.erase(std::remove(old.begin(), old.end(), s), old.end());
    b->stream_width[(size_t)s] = w;
    b->groups[(size_t)w].streams.push_back(s);
  }
  std::sort(b->groups[(size_t)w].streams.begin(), b->groups[(size_t)w].streams.end());
  int rc = ensure_state(b, b->groups[(size_t)w]);
  for (size_t i = 0; rc == NAM_HIP_OK && i < b->groups.size(); i++)
    rc = refresh_map(b, b->groups[i]);
  return rc;
}

// ---- a container's batch at mixed sizes in persistent mode (api_internal.h: SizeMix) ----

// The two residencies' rules (api_internal.h: MixFamilyRules); the functions below ask this table and name no family
const MixFamilyRules kMixFamily[MIX_FAMILY_COUNT] = {
  {"A2", PERSIST_KQ, NAM_HIP_KERNEL_A1_MFMA, NAM_HIP_KERNEL_WN_REG, 1u << FN_KQ | 1u << FN_KT_MFMA,
   "A2 container at mixed sizes in persistent mode: only nam_kq_kernel and nam_kt_mfma_kernel run it "
   "(a launch beyond 2^28 frames would take nam_a1_kernel: split the launch)",
   BANK_BLOB_WHOLE, MIX_MOVE_TRANSCODE, "nam_a2_transcode_kernel"},
  {"A1", PERSIST_A1_P2, NAM_HIP_KERNEL_A1_IL, NAM_HIP_KERNEL_A1_IL, 1u << FN_A1_P2 | 1u << FN_A1_P4 | 1u << FN_A1_Q,
   "A1 container at mixed sizes in persistent mode: only the interleaved-frame kernels (nam_a1_q_kernel, nam_a1_p4_kernel, "
   "nam_a1_p2_kernel) run it",
   BANK_BLOB_KERNEL_REGION, MIX_MOVE_COPY, "nam_state_rows_copy_kernel"},
};

// the plan whose blob is submodel w's member of the device image: the largest submodel's own, a padded second plan, or the submodel's own
static const Plan& mix_member_plan(const nam_hip_model& m, size_t w)
{
  return ((int)w == m.full_width || m.padded.empty()) ? m.plans[w] : m.padded[w];
}

bool mix_wanted(const nam_hip_batch* b)
{
  const nam_hip_model& m = *b->model;
  if (!b->ps.enabled || b->bank || m.mix_family == MIX_NONE)
    return false;
  const MixFamilyRules& r = kMixFamily[m.mix_family];
  const WidthGroup& full = b->groups[(size_t)m.full_width];
  // what persist_kind asks of a one-size batch on the family's session kernel, of the largest submodel's plan over EVERY stream
  if (wavenet_persist_kind(b, full) != r.persist)
    return false;
  if (full.state_family != STATE_FRESH && full.state_family != state_family_of(*full.plan, r.kernel_class))
    return false;
  int sizes = 0;
  for (size_t w = 0; w < b->groups.size(); w++)
  {
    const WidthGroup& g = b->groups[w];
    if (g.streams.empty())
      continue;
    sizes++;
    if ((int)w == m.full_width)
      continue;
    // a narrow stream comes from and goes back to the layout of what its group runs outside the session
    const StateFamily own = state_family_of(*g.plan, r.narrow_class);
    if (!g.d_state || state_family_of(*g.plan, pick_kernel(b, g)) != own || (g.state_family != STATE_FRESH && g.state_family != own))
      return false;
    if (r.move == MIX_MOVE_TRANSCODE && !m.transcode[w].ok)
      return false;
    if (r.move == MIX_MOVE_COPY && g.plan->state_floats != full.plan->state_floats)
      return false;
  }
  return sizes > 1;
}

// the device side of SizeMix, once per batch (a control call: set_persistent, set_slimmable_size ... allocate, process calls never)
static int mix_prepare(nam_hip_batch* b)
{
  SizeMix& mx = b->mix;
  if (mx.d_blob)
    return NAM_HIP_OK;
  const nam_hip_model& m = *b->model;
  const MixFamilyRules& r = mix_rules(b);
  const Plan& full = m.plans[(size_t)m.full_width];
  const size_t n = m.plans.size();
  const size_t region = full.blob.size() - (size_t)mix_blob_base(full, r);
  const size_t stride = (region + 3) / 4 * 4; // (the kernels read 16-byte records)
  std::vector<float> blobs(n * stride, 0.0f), scal(2 * n, 0.0f);
  DeviceBuf<float> d_blob, d_scal;
  DeviceBuf<int> d_member;
  std::vector<DeviceBuf<A2XcRing>> d_rings(n);
  for (size_t w = 0; w < n; w++)
  {
    const Plan& p = mix_member_plan(m, w);
    const int base = mix_blob_base(p, r);
    if (base < 0 || (size_t)base > p.blob.size() || p.blob.size() - (size_t)base != region)
      return fail(NAM_HIP_ERR_MODEL, "container at mixed sizes: a submodel's blob does not have the largest submodel's size");
    std::memcpy(blobs.data() + w * stride, p.blob.data() + base, region * sizeof(float));
    scal[2 * w] = p.blob[(size_t)p.a1.head_scale_off];
    // (as a bank's members, api_bank.cpp: nam_kq_kernel runs ReLU as LeakyReLU with slope 0)
    scal[2 * w + 1] = (r.persist == PERSIST_KQ && p.a1.arr[0].act == ACT_RELU) ? 0.0f : p.a1.arr[0].act_p0;
    if ((int)w == m.full_width || r.move != MIX_MOVE_TRANSCODE)
      continue;
    const A2Transcode& t = m.transcode[w];
    // the table against the rows it will be run on (a2_transcode_check has walked it at load: build_model)
    if (t.wr_state_floats > m.plans[w].state_floats || t.a2_state_floats > full.state_floats)
      return fail(NAM_HIP_ERR_MODEL, "A2 container: the transcode table names floats outside the state rows");
    NAM_HIP_CHECK(upload(d_rings[w], t.rings.data(), t.rings.size()));
  }
  NAM_HIP_CHECK(upload(d_blob, blobs.data(), blobs.size()));
  NAM_HIP_CHECK(upload(d_scal, scal.data(), scal.size()));
  NAM_HIP_CHECK(hipMalloc(d_member.out(), (size_t)b->n_streams * sizeof(int)));
  mx.d_blob = std::move(d_blob); // (all or nothing)
  mx.d_scal = std::move(d_scal);
  mx.d_member = std::move(d_member);
  mx.d_rings = std::move(d_rings);
  mx.stride = (long)stride;
  return NAM_HIP_OK;
}

// the streams `d_streams` (device memory, n of them) of the narrow group `w` between its own rows and the largest submodel's, by the
// family's mover, on the batch's stream
static int mix_move(nam_hip_batch* b, size_t w, const int* d_streams, int n, bool to_resident)
{
  const nam_hip_model& m = *b->model;
  WidthGroup& full = b->groups[(size_t)m.full_width];
  WidthGroup& g = b->groups[w];
  if (!d_streams || !g.d_state || !full.d_state)
    return fail(NAM_HIP_ERR_MODEL, "container at mixed sizes: a narrow group without a stream list or state");
  if (mix_rules(b).move == MIX_MOVE_TRANSCODE)
    NAM_HIP_CHECK(launch_a2_transcode(b->mix.d_rings[w].get(), (int)m.transcode[w].rings.size(), full.d_state.get(), full.state_stride, g.d_state.get(),
                                      g.state_stride, d_streams, n, to_resident, b->stream.get()));
  else
  {
    // (mix_wanted: the two plans' rows have one size; a row is state_stride >= state_floats floats on either side)
    if (g.plan->state_floats != full.plan->state_floats || g.state_stride < g.plan->state_floats || full.state_stride < full.plan->state_floats)
      return fail(NAM_HIP_ERR_MODEL, "container at mixed sizes: a narrow group's state rows are not the largest submodel's size");
    float* const own = g.d_state.get();
    float* const res = full.d_state.get();
    NAM_HIP_CHECK(launch_state_rows_copy(to_resident ? res : own, to_resident ? full.state_stride : g.state_stride, to_resident ? own : res,
                                         to_resident ? g.state_stride : full.state_stride, d_streams, n, g.plan->state_floats, b->stream.get()));
  }
  b->mix.n_moves++;
  b->mix.n_streams_moved += (unsigned long long)n;
  return NAM_HIP_OK;
}

// every narrow stream's state between its group's row and the largest submodel's, on the batch's stream (the batch is quiesced)
static int mix_move_all(nam_hip_batch* b, bool to_resident)
{
  const nam_hip_model& m = *b->model;
  const double t0 = stats_on() ? stat_now_us() : 0.0;
  for (size_t w = 0; w < b->groups.size(); w++)
  {
    WidthGroup& g = b->groups[w];
    if ((int)w == m.full_width || g.streams.empty())
      continue;
    // (a narrow group of a mixed batch never holds every stream: refresh_map has given it its stream list)
    if (const int rc = mix_move(b, w, g.d_map.get(), (int)g.streams.size(), to_resident))
      return rc;
  }
  NAM_HIP_CHECK(hipStreamSynchronize(b->stream.get()));
  if (stats_on())
    b->mix.t_move_us += stat_now_us() - t0;
  return NAM_HIP_OK;
}

int mix_enter(nam_hip_batch* b)
{
  if (b->mix.resident)
    return NAM_HIP_OK;
  NAM_HIP_CHECK(quiesce(b));
  if (const int rc = mix_prepare(b))
    return rc;
  NAM_HIP_CHECK(hipMemcpy(b->mix.d_member.get(), b->stream_width.data(), (size_t)b->n_streams * sizeof(int), hipMemcpyHostToDevice));
  if (const int rc = mix_move_all(b, true))
    return rc;
  const nam_hip_model& m = *b->model;
  const MixFamilyRules& r = mix_rules(b);
  for (size_t w = 0; w < b->groups.size(); w++)
  {
    WidthGroup& g = b->groups[w];
    if (g.streams.empty())
      continue;
    // zeros are zeros in either layout; from here on the rows are what they were moved as
    if (g.state_family == STATE_FRESH)
      g.state_family = state_family_of(*g.plan, (int)w == m.full_width ? r.kernel_class : r.narrow_class);
  }
  b->mix.resident = true;
  return NAM_HIP_OK;
}

int mix_leave(nam_hip_batch* b)
{
  if (!b->mix.resident)
    return NAM_HIP_OK;
  NAM_HIP_CHECK(quiesce(b));
  if (const int rc = mix_move_all(b, false))
    return rc;
  b->mix.resident = false;
  return NAM_HIP_OK;
}

int mix_sync(nam_hip_batch* b)
{
  return mix_wanted(b) ? mix_enter(b) : mix_leave(b);
}

// ---- stream slots (include/nam_hip.h: nam_hip_batch_restart_streams, _get / _set_stream_state) ----

uint64_t model_fingerprint(const ModelSpec& s)
{
  uint64_t h = sstate::fnv1a64(s.architecture_name.data(), s.architecture_name.size());
  h = sstate::fnv1a64(s.config_text.data(), s.config_text.size(), h);
  const int32_t flags[2] = {s.arch, s.fast_tanh ? 1 : 0};
  h = sstate::fnv1a64(flags, sizeof(flags), h);
  if (const std::vector<float>* w = s.weights())
    h = sstate::fnv1a64(w->data(), w->size() * sizeof(float), h);
  auto nested = [&](const ModelSpec& sub) {
    const uint64_t f = model_fingerprint(sub);
    h = sstate::fnv1a64(&f, sizeof(f), h);
  };
  if (s.arch == ARCH_WAVENET && s.wavenet.condition_dsp)
    nested(*s.wavenet.condition_dsp);
  for (const auto& sub : s.submodels)
    nested(*sub);
  return h;
}

// The state of a newly created batch after nam_hip_batch_reset(prewarm), for the streams `ids` (ascending, unique, in range)
static int restart_streams_in_groups(nam_hip_batch* b, const std::vector<int>& ids, bool prewarm);
int restart_streams(nam_hip_batch* b, const std::vector<int>& ids, bool prewarm)
{
  NAM_HIP_CHECK(quiesce(b));
  // (a container at mixed sizes: every stream back in its own group's rows, the restart as ever, the batch resident again)
  if (const int rc = mix_leave(b))
    return rc;
  if (const int rc = restart_streams_in_groups(b, ids, prewarm))
    return rc;
  return mix_sync(b);
}
static int restart_streams_in_groups(nam_hip_batch* b, const std::vector<int>& ids, bool prewarm)
{
  if (b->lin.on) // the streams' columns of the one ring; sizes, the position and every other column stay
  {
    for (int s : ids)
      NAM_HIP_CHECK(launch_linear_stream_cols(b->lin.d_hist.get(), b->lin.hist_frames, b->lin.caps.cols_pad, b->lin.pos, s, 1, nullptr,
                                              LINEAR_COLS_ZERO, b->stream.get()));
    NAM_HIP_CHECK(hipStreamSynchronize(b->stream.get()));
    return NAM_HIP_OK;
  }
  for (size_t w = 0; w < b->groups.size(); w++)
  {
    WidthGroup& g = b->groups[w];
    std::vector<int> sub; // the listed streams of this group (a slimmable stream keeps its width)
    for (int s : ids)
      if (b->stream_width[(size_t)s] == (int)w)
        sub.push_back(s);
    if (sub.empty())
      continue;
    const Plan& p = *g.plan;
    if (p.arch == ARCH_LINEAR) // the stream's own columns of the shared ring; the position and every other column stay
    {
      const int cps = p.linear.cols_per_stream;
      for (int s : sub)
        NAM_HIP_CHECK(launch_linear_stream_cols(g.d_lin_hist.get(), g.lin_hist_frames, g.lin_cols_pad, g.lin_pos, s * cps, cps, nullptr,
                                                LINEAR_COLS_ZERO, b->stream.get()));
      NAM_HIP_CHECK(hipStreamSynchronize(b->stream.get()));
      continue;
    }
    const bool all = sub.size() == g.streams.size();
    DeviceBuf<int> d_sub;
    if (!all)
      NAM_HIP_CHECK(upload(d_sub, sub.data(), sub.size()));
    const int* const d_map = all ? g.d_map.get() : d_sub.get();
    int rc = NAM_HIP_OK;
    // an LSTM's Reset clears nothing (nam_hip_batch_reset mirrors the reference): a new player's slot gets h0 / c0 first, as a
    // newly created batch's streams do (ensure_state)
    if (p.arch == ARCH_LSTM && g.d_bank_member)
      rc = bank_fill_initial_state(b, g, d_map, (int)sub.size());
    else if (p.arch == ARCH_LSTM)
    {
      const hipError_t e = launch_fill_state(g.d_state.get(), g.state_stride, d_map, (int)sub.size(), g.d_init.get(), (int)p.lstm.init_state.size(),
                                             p.state_floats, b->stream.get());
      if (e != hipSuccess)
        rc = fail(NAM_HIP_ERR_DEVICE, std::string("launch_fill_state: ") + hipGetErrorString(e));
    }
    if (rc == NAM_HIP_OK)
      rc = reset_streams(b, g, d_map, (int)sub.size(), prewarm, sub.front());
    const hipError_t e = hipStreamSynchronize(b->stream.get()); // (before d_sub goes: the launches read it)
    if (rc != NAM_HIP_OK)
      return rc;
    NAM_HIP_CHECK(e);
  }
  return NAM_HIP_OK;
}

// the history ring a Linear stream's columns live in: the group's own, or the one ring of an all-Linear container's batch
struct LinRing
{
  float* hist;
  int frames, cols_pad, pos;
};
static LinRing lin_ring(const nam_hip_batch* b, const WidthGroup& g)
{
  if (b->lin.on)
    return LinRing{b->lin.d_hist.get(), b->lin.hist_frames, b->lin.caps.cols_pad, b->lin.pos};
  return LinRing{g.d_lin_hist.get(), g.lin_hist_frames, g.lin_cols_pad, g.lin_pos};
}

// what the plan of width `w` keeps per stream and what its group holds now (stream_state.h)
static sstate::Geometry stream_geometry(const nam_hip_batch* b, int w)
{
  const WidthGroup& g = b->groups[(size_t)w];
  const Plan& p = *g.plan;
  sstate::Geometry q;
  q.arch = p.arch;
  if (p.arch == ARCH_LINEAR)
  {
    q.lin_hist_frames = lin_ring(b, g).frames;
    q.lin_channels = p.linear.cols_per_stream;
    return q;
  }
  q.state_floats = p.state_floats;
  if (p.arch == ARCH_WAVENET)
  {
    q.state_family = (int32_t)g.state_family;
    q.layout0 = p.wr.ok ? p.wr.hist_floats : 0;
    q.layout1 = p.wr.ok ? p.wr.n_layers : 0;
  }
  else
  {
    q.layout0 = p.lstm.hidden;
    q.layout1 = p.lstm.n_layers;
  }
  return q;
}
static_assert(sstate::kFamilyFresh == (int)STATE_FRESH && (int)STATE_WN_REG == 2, "stream_state.h validates StateFamily's range");
static_assert(ARCH_LINEAR == 4, "stream_state.h: Geometry::payload_bytes");

int64_t stream_state_bytes(const nam_hip_batch* b, int stream)
{
  return sstate::blob_bytes(stream_geometry(b, b->stream_width[(size_t)stream]));
}

int get_stream_state(nam_hip_batch* b, int stream, void* buf)
{
  NAM_HIP_CHECK(quiesce(b));
  const int w = b->stream_width[(size_t)stream];
  WidthGroup& g = b->groups[(size_t)w];
  const sstate::Geometry q = stream_geometry(b, w);
  const size_t bytes = (size_t)q.payload_bytes();
  std::vector<float> payload(bytes / sizeof(float));
  if (b->mix.resident && w != b->model->full_width)
  {
    // the stream lives zero-padded in the largest submodel's rows (SizeMix): its blob is its own group's row, as ever — this one
    // stream's rings are copied there first (the padded copy stays the live one; no other stream is touched)
    DeviceBuf<int> d_one;
    NAM_HIP_CHECK(upload(d_one, &stream, 1));
    const double t0 = stats_on() ? stat_now_us() : 0.0;
    const int rm = mix_move(b, (size_t)w, d_one.get(), 1, false);
    const hipError_t es = hipStreamSynchronize(b->stream.get()); // (before `d_one` goes)
    if (rm != NAM_HIP_OK)
      return rm;
    NAM_HIP_CHECK(es);
    if (stats_on())
      b->mix.t_move_us += stat_now_us() - t0;
  }
  if (q.arch == ARCH_LINEAR)
  {
    DeviceBuf<float> rows; // the stream's columns, oldest frame first
    NAM_HIP_CHECK(hipMalloc(rows.out(), bytes));
    const LinRing r = lin_ring(b, g);
    hipError_t e = launch_linear_stream_cols(r.hist, r.frames, r.cols_pad, r.pos, stream * q.lin_channels, q.lin_channels, rows.get(),
                                             LINEAR_COLS_GATHER, b->stream.get());
    if (e == hipSuccess)
      e = hipMemcpyAsync(payload.data(), rows.get(), bytes, hipMemcpyDeviceToHost, b->stream.get());
    const hipError_t es = hipStreamSynchronize(b->stream.get()); // (before `rows` goes)
    NAM_HIP_CHECK(e);
    NAM_HIP_CHECK(es);
  }
  else
  {
    NAM_HIP_CHECK(hipMemcpyAsync(payload.data(), g.d_state.get() + (size_t)stream * g.state_stride, bytes, hipMemcpyDeviceToHost, b->stream.get()));
    NAM_HIP_CHECK(hipStreamSynchronize(b->stream.get()));
  }
  const int member = b->bank ? b->stream_member[(size_t)stream] : -1;
  sstate::encode(buf, b->bank ? b->bank->fingerprint : model_fingerprint(*b->model->spec), member,
                 b->bank ? b->bank->member_fp[(size_t)member] : 0, w, q, payload.data());
  return NAM_HIP_OK;
}

static int set_stream_state_in_groups(nam_hip_batch* b, int stream, const void* buf, int64_t size);
int set_stream_state(nam_hip_batch* b, int stream, const void* buf, int64_t size)
{
  NAM_HIP_CHECK(quiesce(b));
  // (a container at mixed sizes: the blob is written into the stream's own group's row with every stream back in its own; what
  // the batch is afterwards — the blob may have changed the stream's size — decides where the streams live from here on)
  if (const int rc = mix_leave(b))
    return rc;
  const int rc = set_stream_state_in_groups(b, stream, buf, size);
  const int rs = mix_sync(b); // (also behind a refusal: the batch goes back to where it was)
  return rc != NAM_HIP_OK ? rc : rs;
}
static int set_stream_state_in_groups(nam_hip_batch* b, int stream, const void* buf, int64_t size)
{
  // 1. everything the blob says against the batch, before anything changes
  std::vector<sstate::Geometry> widths;
  for (size_t w = 0; w < b->groups.size(); w++)
    widths.push_back(stream_geometry(b, (int)w));
  sstate::Expect ex;
  ex.model_fp = b->bank ? b->bank->fingerprint : model_fingerprint(*b->model->spec);
  ex.member_fp = b->bank ? b->bank->member_fp.data() : nullptr;
  ex.n_members = b->bank ? b->bank->n_members : 0;
  ex.widths = widths.data();
  ex.n_widths = (int32_t)widths.size();
  sstate::Header h;
  const std::string why = sstate::validate(buf, size, ex, h);
  if (!why.empty())
    return fail(NAM_HIP_ERR_INVALID_ARGUMENT, "nam_hip_batch_set_stream_state: " + why);
  const float* const payload = reinterpret_cast<const float*>(static_cast<const char*>(buf) + sizeof(sstate::Header));
  // 2. the stream joins the blob's width group, as nam_hip_batch_set_slimmable_size moves it — without the reset
  if (b->stream_width[(size_t)stream] != h.width)
  {
    const int rc = b->lin.on ? lin_container_move(b, {stream}, h.width, false) : move_streams_to_width(b, {stream}, h.width);
    if (rc != NAM_HIP_OK)
      return rc;
  }
  WidthGroup& g = b->groups[(size_t)h.width];
  // 3. ... and is bound to the blob's member
  if (b->bank && b->stream_member[(size_t)stream] != h.member)
  {
    b->stream_member[(size_t)stream] = h.member;
    NAM_HIP_CHECK(hipMemcpy(g.d_bank_member.get(), b->stream_member.data(), (size_t)b->n_streams * sizeof(int), hipMemcpyHostToDevice));
  }
  // 4. the state
  const size_t bytes = (size_t)h.payload_bytes;
  if (h.arch == ARCH_LINEAR)
  {
    DeviceBuf<float> rows; // oldest frame first: rotated to this batch's ring position by the kernel
    NAM_HIP_CHECK(upload(rows, payload, bytes / sizeof(float)));
    const LinRing r = lin_ring(b, g);
    const hipError_t e = launch_linear_stream_cols(r.hist, r.frames, r.cols_pad, r.pos, stream * h.lin_channels, h.lin_channels, rows.get(),
                                                   LINEAR_COLS_SCATTER, b->stream.get());
    const hipError_t es = hipStreamSynchronize(b->stream.get()); // (before `rows` goes)
    NAM_HIP_CHECK(e);
    NAM_HIP_CHECK(es);
    return NAM_HIP_OK;
  }
  NAM_HIP_CHECK(hipMemcpyAsync(g.d_state.get() + (size_t)stream * g.state_stride, payload, bytes, hipMemcpyHostToDevice, b->stream.get()));
  NAM_HIP_CHECK(hipStreamSynchronize(b->stream.get()));
  if (h.arch == ARCH_WAVENET && g.state_family == STATE_FRESH) // (the other streams of the group are zeros: any layout's)
    g.state_family = (StateFamily)h.state_family;
  return NAM_HIP_OK;
}

int build_model(std::shared_ptr<ModelSpec> spec, nam_hip_model** out)
{
  auto m = std::make_unique<nam_hip_model>();
  m->spec = std::move(spec);
  // layer shapes outside nam_wn_reg_kernel's ahead-of-time tables: collected over every plan of the model (the widths of
  // a slimmable WaveNet, the submodels of a container) and compiled as ONE code object (wr_jit.cpp), so that a batch with
  // mixed widths still runs as one launch
  WrShapeSet jit_shapes;
  WrShapeSet* const js = wr_jit_enabled() ? &jit_shapes : nullptr;
  if (m->spec->arch == ARCH_WAVENET && m->spec->wavenet.slimmable)
  {
    // enumerate the distinct widths: one probe ratio per interval between breakpoints
    std::vector<double> bp = slimmable_breakpoints(m->spec->wavenet);
    std::vector<double> probes;
    double lo = 0.0;
    for (double x : bp)
    {
      probes.push_back(0.5 * (lo + x));
      lo = x;
    }
    probes.push_back(0.5 * (lo + 1.0));
    probes.push_back(1.0);
    for (double r : probes)
    {
      const std::vector<int> ch = channels_for_ratio(m->spec->wavenet, r);
      if (std::find(m->width_channels.begin(), m->width_channels.end(), ch) == m->width_channels.end())
      {
        m->width_channels.push_back(ch);
        m->plans.push_back(build_wavenet_plan(slim_wavenet(m->spec->wavenet, ch), js));
      }
    }
    m->full_width = m->width_for_ratio(1.0);
  }
  else if (m->spec->arch == ARCH_CONTAINER)
  {
    // one plan per submodel (a slimmable submodel stays at its full size: ContainerModel never forwards
    // SetSlimmableSize to its children); a fresh container has the last submodel active (container.cpp:49)
    for (const auto& sm : m->spec->submodels)
    {
      m->plans.push_back(build_plan(*sm, js));
      m->width_channels.push_back({});
    }
    m->full_width = (int)m->plans.size() - 1;
  }
  else
  {
    m->plans.push_back(build_plan(*m->spec, js));
    m->width_channels.push_back({});
    m->full_width = 0;
  }
  bool any_jit = false;
  for (const Plan& p : m->plans)
    any_jit = any_jit || (p.wr.ok && p.wr.jit);
  if (any_jit)
  {
    std::string why;
    const std::string module = wr_jit_build(jit_shapes, why);
    const std::string masked = jit_shapes.header_text(true); // (WrPlan::structure_key: the code object's text but for the scales)
    for (size_t i = 0; i < m->plans.size(); i++)
    {
      Plan& p = m->plans[i];
      if (!(p.wr.ok && p.wr.jit))
        continue;
      if (!module.empty())
      {
        p.wr.jit_module = module;
        p.wr.structure_key = wr_hash(masked.data(), masked.size(), p.wr.structure_key);
      }
      else
      {
        // no compiler / sources here: plan again without the model's own shapes (run-time-flag instantiations if the
        // model fits them, else the other kernels take it)
        const ModelSpec& sp = m->spec->arch == ARCH_CONTAINER ? *m->spec->submodels[i] : *m->spec;
        Plan again = (sp.arch == ARCH_WAVENET && sp.wavenet.slimmable) ? build_wavenet_plan(slim_wavenet(sp.wavenet, m->width_channels[i]))
                                                                       : build_plan(sp);
        if (!again.wr.ok)
          again.wr.why += " [" + why + "]";
        // loud: the model still runs, but off its compiled shapes (run-time-flag instantiations, or another kernel: 6 - 9 x
        // slower, profiles/r03/defit_table.txt). nam_hip_model_info says so (has_a1_kernel bit 5), the description too.
        again.wr.jit_failed = why.empty() ? "unknown reason" : why;
        std::fprintf(stderr, "libnam_hip: %s: nam_wn_reg_kernel could not be compiled for this model's layer shapes (%s); it runs on %s\n",
                     sp.architecture_name.c_str(), again.wr.jit_failed.c_str(),
                     again.wr.ok ? "the run-time-flag instantiations" : "another kernel");
        p = std::move(again);
      }
    }
  }
  // a container on the A2 family (nam_hip_model::padded): every narrower submodel zero-padded onto the largest one's layout, and
  // the table between its two residences, walked once here. All or nothing: one submodel without its pair and a batch at mixed
  // sizes stays what it was, a launch per size and no session.
  if (m->spec->arch == ARCH_CONTAINER && m->plans.size() > 1 && m->plans[(size_t)m->full_width].arch == ARCH_WAVENET)
  {
    const Plan& full = m->plans[(size_t)m->full_width];
    std::vector<Plan> padded(m->plans.size());
    std::vector<A2Transcode> transcode(m->plans.size());
    bool all = full.a1.valid && full.a1.kt_ok && full.a1.kp_ok;
    for (size_t w = 0; all && w < m->plans.size(); w++)
    {
      if ((int)w == m->full_width)
        continue;
      const ModelSpec& sm = *m->spec->submodels[w];
      std::string why;
      all = sm.arch == ARCH_WAVENET && m->plans[w].arch == ARCH_WAVENET && build_a2_padded_plan(sm.wavenet, full, padded[w], why);
      if (all)
      {
        transcode[w] = build_a2_transcode(m->plans[w], padded[w]);
        all = transcode[w].ok && a2_transcode_check(transcode[w]).empty() && transcode[w].wr_state_floats <= m->plans[w].state_floats
              && transcode[w].a2_state_floats <= full.state_floats;
      }
    }
    if (all)
    {
      m->padded = std::move(padded);
      m->transcode = std::move(transcode);
      m->mix_family = MIX_A2;
    }
    else if (full.a1.valid && full.a1.il_ok && full.a1.p2_ok)
    {
      // ... or on the official WaveNet topology (standard, lite, feather): the submodels as they are planned — zero-padded to
      // 16 / 8 in the padded ring layout — are members of one BANK_A1_IL bank, or the container has no residency. Asked of
      // the bank's own rules (api_bank.cpp), once, here.
      const std::string why = container_a1_difference(*m);
      if (why.empty())
        m->mix_family = MIX_A1;
      m->mix_note = why.empty() ? "a1_mixed_session=1 (every submodel is the official topology at padded 16 / 8 channels: a batch at mixed "
                                  "sizes runs persistent mode as one session of nam_a1_q_kernel)"
                                : "a1_mixed_session=0 (" + why + ": a batch at mixed sizes runs a launch per size and no session)";
    }
  }
  *out = m.release();
  return NAM_HIP_OK;
}

} // namespace api
} // namespace namhip
