// api_bank.cpp — model banks (include/nam_hip.h: nam_hip_bank_create, nam_hip_batch_create_bank): which models may share a
// batch, the bank's host image, a bank batch's device image and the per-stream member binding. See api_internal.h.
//
// A bank is of ONE family (BankFamily), decided by member 0:
//  * BANK_A1_IL: the official WaveNet topology on the interleaved-frame kernels. What the bank holds per member is the part of
//    the plan's blob those kernels read — from A1Plan::ws_tiles_off to the end: tiles | extra tiles | constants | rechannel column
//    | nam_a1_q_kernel's weight block. In front of that region a plan keeps the op program's weights in the model's OWN channel
//    counts, so the region starts at another offset in a lite or feather model than in a standard one; inside it the layout is
//    the padded 16 / 8 topology's and the same for every member. The launch arguments of such a bank batch are therefore offsets
//    from the region's start (launch_group), and the comparison below is made on those.
//  * BANK_A2: the A2 topology (kp_table.h) on nam_kq_kernel / nam_kt_mfma_kernel. Every member has the same channel counts, so
//    the WHOLE blob has one layout: the bank keeps whole blobs (base offset 0) and A1Plan's absolute offsets (kt_desc[].tile_off,
//    kt_rech_off, kt_lds_src_off, kq_w_off) hold against any member's row.
//  * BANK_LSTM: LSTMs of one shape on nam_lstm_row_kernel (hidden <= 4) / nam_lstm_wide_kernel (5 .. 32 units). Whole blobs again
//    (base offset 0): LSTMPlan's absolute offsets (layer_w[], layer_b[], head_w, head_b) hold against any member's row. No A1Plan,
//    no scalars; instead every member's initial state (h0 / c0 are part of an LSTM's weight stream: LSTMPlan::init_state).
//  * BANK_WN_REG: WaveNets that a one-model batch runs on nam_wn_reg_kernel under AUTO — the official nano size, FiLM, gating, a
//    nested condition_dsp, a post-stack head, narrow plain stacks — of ONE program: equal WrPlan::structure_key. The bank keeps
//    WrPlan::blob whole (weights | tables | op program; base offset 0), and nothing besides: head_scale and a nested condition's
//    scale are in the member's own op table, where a bank launch reads them (kernel_wn_reg.hip: wr_scales) — a per-model code
//    object has them compiled in, so two captures of one topology have two code objects; the launch runs member 0's (the proto
//    plan's) and a member's own, which its load compiled, stays unused. Such a bank runs nam_wn_reg_kernel at EVERY stream count:
//    a one-model batch of a plain narrow model beyond kPersistTurns x per_cu x CUs streams flips to nam_a1_kernel and another
//    state layout (pick_kernel), the bank does not (beyond that count it has no session: a launch per buffer).
// Per member besides the blob, the two A1Plan families: the two scalars the kernels take by value (head_scale, act_p0 — on the A2
// topology the LeakyReLU slope, 0 for ReLU as in launch_kq).
//
// A family's rules are its row of kBankFamily below (api_internal.h: BankFamilyRules); the other files ask that row and name no
// family. Here a family is named by member_refusal (which family a model is of), by its comparison function and by its row.
#include "api_internal.h"

#include <cstdio>

namespace namhip
{
namespace api
{
namespace
{
// What a model stands for in a bank: its full-size plan and that plan's spec (a SlimmableContainer: its largest submodel's, the
// one a batch runs when no size has been set).
const Plan& member_plan(const nam_hip_model& m)
{
  return m.plans[m.full_width];
}
std::shared_ptr<ModelSpec> member_spec(const nam_hip_model& m)
{
  return m.spec->arch == ARCH_CONTAINER ? m.spec->submodels[(size_t)m.full_width] : m.spec;
}
// the A2 family: what makes a one-model batch session-eligible on nam_kq_kernel (kq_runs), nam_kt_mfma_kernel for a lone buffer
bool a2_member(const A1Plan& a)
{
  return a.valid && a.kt_ok && a.kp_ok && kq_takes(a.arr[0].act, a.arr[0].act_p0);
}

// Why `m` cannot be a bank member at all ("" = it can, and *family says of which family).
std::string member_refusal(const nam_hip_model& m, int* family)
{
  const ModelSpec& s = *m.spec;
  *family = BANK_A1_IL;
  if (s.arch == ARCH_LINEAR)
    return "a Linear model (nam_linear_kernel multiplies ONE shared impulse response with every stream's history; per-stream "
           "impulse responses are another kernel: no bank family takes it)";
  if (s.arch == ARCH_LSTM)
  {
    const LSTMPlan& L = member_plan(m).lstm;
    if (!(lstm_row_eligible(L) || lstm_wide_eligible(L)))
      return "an LSTM outside nam_lstm_row_kernel / nam_lstm_wide_kernel (hidden " + std::to_string(L.hidden) + ", "
             + std::to_string(L.n_layers) + " layer(s), input_size " + std::to_string(L.input_size)
             + ": more than 32 hidden units, more than two layers or more than two inputs run on nam_lstm_mfma_kernel / "
               "nam_lstm_kernel, whose streams share one wavefront's weights: they know no banks)";
    *family = BANK_LSTM;
    return "";
  }
  if (s.arch == ARCH_CONTAINER)
  {
    // a container stands for its largest submodel, and only in the A2 family (how A2 captures ship)
    if (m.plans.empty() || member_spec(m)->arch != ARCH_WAVENET || !a2_member(member_plan(m).a1))
      return "a SlimmableContainer whose largest submodel is not an A2-topology WaveNet on nam_kq_kernel (kt_ok / kp_ok / kq_takes)";
    *family = BANK_A2;
    return "";
  }
  if (m.slimmable())
    return "a slimmable WaveNet (its widths are separate plans; banks hold one plan per member)";
  const Plan& p = member_plan(m);
  const A1Plan& a = p.a1;
  // pick_kernel's AUTO answer for a one-model batch (below the stream count at which a plain narrow model flips to nam_a1_kernel)
  if (p.wr.ok && !(a.valid && (a.ws_ok || a.kt_ok)))
  {
    *family = BANK_WN_REG;
    return "";
  }
  if (!a.valid)
    return "outside the A1 kernel family (FiLM / gating / groups / a lookup-table or per-channel activation / a post-stack head ...) and "
           "without a nam_wn_reg_kernel plan ("
           + (p.wr.jit_failed.empty() ? p.wr.why : p.wr.why + "; per-model compile: " + p.wr.jit_failed) + ")";
  if (a2_member(a))
  {
    *family = BANK_A2;
    return "";
  }
  if (a.kt_ok && a.kp_ok)
    return "the A2 topology with an activation nam_kq_kernel is not compiled for (kq_takes: LeakyReLU with a slope <= 1, ReLU, Tanh, Fasttanh)";
  if (!(a.il_ok && a.p2_ok && a.q_ok && a.p2_c0 == 16 && a.p2_c1 == 8))
    return "neither the official WaveNet topology at (padded) 16 / 8 channels with Tanh or Fasttanh (no nam_a1_q_kernel plan: q_ok / "
           "p2_c0 / p2_c1) nor the A2 topology (no nam_kq_kernel plan: kt_ok / kp_ok)";
  if (!a1_q_takes(a.arr[0].act))
    return "an activation nam_a1_q_kernel is not compiled for (arr[0].act)";
  if (a.ws_tiles_off % 4 != 0 || a.ws_consts_off < a.ws_tiles_off || a.ws_xt_off < a.ws_tiles_off || a.q_w_off < a.ws_tiles_off
      || (size_t)a.ws_tiles_off >= p.blob.size())
    return "a blob layout whose kernel region does not start at its tile area (ws_tiles_off)";
  return "";
}

// The comparisons below: member `m` against member 0, field by field. The recorder keeps the FIRST field that differs (what a
// refusal names); "" = the two run as one launch.
struct FirstDifference
{
  std::string text;
  void operator()(const char* field, long long x, long long y)
  {
    if (text.empty() && x != y)
      text = std::string(field) + " (" + std::to_string(x) + " vs " + std::to_string(y) + ")";
  }
};

// both WaveNet families: channels, prewarm, state, the arrays and their rings
void wavenet_geometry(FirstDifference& cmp, const Plan& p, const Plan& q)
{
  const A1Plan &a = p.a1, &b = q.a1;
  cmp("in_channels", p.in_channels, q.in_channels);
  cmp("out_channels", p.out_channels, q.out_channels);
  cmp("prewarm_samples", p.prewarm_samples, q.prewarm_samples);
  cmp("state_floats", p.state_floats, q.state_floats);
  cmp("a1.n_arrays", a.n_arrays, b.n_arrays);
  cmp("a1.n_rings", a.n_rings, b.n_rings);
  for (int r = 0; r < 64 && r < a.n_rings; r++)
    cmp("a1.ring_len_by_id", a.ring_len_by_id[r], b.ring_len_by_id[r]);
  for (int i = 0; i < a.n_arrays && i < kA1MaxArrays; i++)
  {
    const A1Array &x = a.arr[i], &y = b.arr[i];
    cmp("a1.arr.act (ACT_T)", x.act, y.act); // (A2: after the fast_tanh rewrite; the slope is per member)
    cmp("a1.arr.channels", x.channels, y.channels);
    cmp("a1.arr.kernel", x.kernel, y.kernel);
    cmp("a1.arr.n_layers", x.n_layers, y.n_layers);
    cmp("a1.arr.head_size", x.head_size, y.head_size);
    for (int l = 0; l < x.n_layers && l < kA1MaxLayers; l++)
    {
      cmp("a1.arr.dil", x.dil[l], y.dil[l]);
      cmp("a1.arr.ring_off", x.ring_off[l], y.ring_off[l]);
      cmp("a1.arr.ring_len", x.ring_len[l], y.ring_len[l]);
      cmp("a1.arr.ring_id", x.ring_id[l], y.ring_id[l]);
    }
  }
}

void a1_il_difference(FirstDifference& cmp, const nam_hip_model& m0, const nam_hip_model& m)
{
  const Plan &p = member_plan(m), &q = member_plan(m0);
  const A1Plan &a = p.a1, &b = q.a1;
  cmp("fast_tanh", m.spec->fast_tanh ? 1 : 0, m0.spec->fast_tanh ? 1 : 0);
  wavenet_geometry(cmp, p, q);
  cmp("a1.p2_c0", a.p2_c0, b.p2_c0);
  cmp("a1.p2_c1", a.p2_c1, b.p2_c1);
  // the launch arguments, as offsets from the kernel region's start (see the head of this file)
  cmp("blob floats behind ws_tiles_off", (long long)p.blob.size() - a.ws_tiles_off, (long long)q.blob.size() - b.ws_tiles_off);
  cmp("consts_off (ws_consts_off - ws_tiles_off)", a.ws_consts_off - a.ws_tiles_off, b.ws_consts_off - b.ws_tiles_off);
  cmp("xt_off (ws_xt_off - ws_tiles_off)", a.ws_xt_off - a.ws_tiles_off, b.ws_xt_off - b.ws_tiles_off);
  cmp("n_xt (ws_n_xt)", a.ws_n_xt, b.ws_n_xt);
  cmp("q_w_off - ws_tiles_off", a.q_w_off - a.ws_tiles_off, b.q_w_off - b.ws_tiles_off);
}

void a2_difference(FirstDifference& cmp, const nam_hip_model& m0, const nam_hip_model& m)
{
  const Plan &p = member_plan(m), &q = member_plan(m0);
  const A1Plan &a = p.a1, &b = q.a1;
  wavenet_geometry(cmp, p, q);
  // what nam_kq_kernel and nam_kt_mfma_kernel take from the plan (the device A1Plan is member 0's), absolute blob offsets
  cmp("blob floats", (long long)p.blob.size(), (long long)q.blob.size());
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
}

void lstm_difference(FirstDifference& cmp, const nam_hip_model& m0, const nam_hip_model& m)
{
  const Plan &p = member_plan(m), &q = member_plan(m0);
  // what nam_lstm_row_kernel / nam_lstm_wide_kernel are instantiated on and what their arguments take from the plan (member 0's)
  const LSTMPlan &x = p.lstm, &y = q.lstm;
  cmp("fast_tanh", x.fast ? 1 : 0, y.fast ? 1 : 0);
  cmp("lstm.n_layers", x.n_layers, y.n_layers);
  cmp("lstm.input_size", x.input_size, y.input_size);
  cmp("lstm.hidden", x.hidden, y.hidden);
  cmp("lstm.in_ch", x.in_ch, y.in_ch);
  cmp("lstm.out_ch", x.out_ch, y.out_ch);
  cmp("lstm.head_w", x.head_w, y.head_w);
  cmp("lstm.head_b", x.head_b, y.head_b);
  for (int l = 0; l < x.n_layers && l < 16; l++)
  {
    cmp("lstm.layer_w", x.layer_w[l], y.layer_w[l]);
    cmp("lstm.layer_b", x.layer_b[l], y.layer_b[l]);
  }
  cmp("blob floats", (long long)p.blob.size(), (long long)q.blob.size());
  cmp("lstm.init_state floats", (long long)x.init_state.size(), (long long)y.init_state.size());
  cmp("prewarm_samples", p.prewarm_samples, q.prewarm_samples); // (half a second at the file's sample rate)
  cmp("state_floats", p.state_floats, q.state_floats);
}

void wr_difference(FirstDifference& cmp, const nam_hip_model& m0, const nam_hip_model& m)
{
  const Plan &p = member_plan(m), &q = member_plan(m0);
  const WrPlan &x = p.wr, &y = q.wr;
  cmp("fast_tanh", m.spec->fast_tanh ? 1 : 0, m0.spec->fast_tanh ? 1 : 0);
  cmp("in_channels", p.in_channels, q.in_channels);
  cmp("out_channels", p.out_channels, q.out_channels);
  cmp("prewarm_samples", p.prewarm_samples, q.prewarm_samples);
  cmp("state_floats", p.state_floats, q.state_floats);
  // the program: op types, shapes, weight offsets, rings, dilations, flags, activations, the tables, the cuts — everything of
  // the plan but the weights and the scales (plan.h). NOT jit_module: another head_scale is another file; the launch runs member 0's
  if (cmp.text.empty() && x.structure_key != y.structure_key)
  {
    char t[96];
    std::snprintf(t, sizeof(t), "wr.structure_key (the program: %016llx vs %016llx)", x.structure_key, y.structure_key);
    cmp.text = t;
  }
  // what launch_wr takes from the plan (member 0's), field by field
  cmp("wr.blob floats", (long long)x.blob.size(), (long long)y.blob.size());
  cmp("wr.n_layers", x.n_layers, y.n_layers);
  cmp("wr.hist_floats", x.hist_floats, y.hist_floats);
  cmp("wr.lds_bytes", x.lds_bytes, y.lds_bytes);
  cmp("wr.tab_rows", x.tab_rows, y.tab_rows);
  cmp("wr.n_rows", x.n_rows, y.n_rows);
  cmp("wr.tab_pf", x.tab_pf, y.tab_pf);
  cmp("wr.n_pf", x.n_pf, y.n_pf);
  cmp("wr.tab_ring", x.tab_ring, y.tab_ring);
  cmp("wr.tab_ops", x.tab_ops, y.tab_ops);
  cmp("wr.n_ops", (long long)x.ops.size(), (long long)y.ops.size());
  for (int i = 0; i < 4; i++)
    cmp("wr.split_op", x.split_op[i], y.split_op[i]);
  cmp("wr.has_layers", x.has_layers ? 1 : 0, y.has_layers ? 1 : 0);
  cmp("wr.has_runs", x.has_runs ? 1 : 0, y.has_runs ? 1 : 0);
  cmp("wr.has_rt_layers", x.has_rt_layers ? 1 : 0, y.has_rt_layers ? 1 : 0);
  cmp("wr.program", x.program, y.program);
  cmp("wr per-model code object (1) / ahead-of-time kernel (0)", x.jit_module.empty() ? 0 : 1, y.jit_module.empty() ? 0 : 1);
}

// ... by family, in kBankFamily's order
void (*const kFirstDifference[BANK_FAMILY_COUNT])(FirstDifference&, const nam_hip_model& m0, const nam_hip_model& m) = {
  a1_il_difference, a2_difference, lstm_difference, wr_difference};
} // namespace

// The families' rules, indexed by BankFamily (api_internal.h: BankFamilyRules); the texts are what a caller reads in nam_hip_last_error
const BankFamilyRules kBankFamily[BANK_FAMILY_COUNT] = {
  {"A1_IL (nam_a1_q_kernel)", NAM_HIP_KERNEL_A1_IL,
   "nam_hip_batch_set_kernel: a bank batch runs the interleaved-frame kernels only (NAM_HIP_KERNEL_AUTO / NAM_HIP_KERNEL_A1_IL)",
   1u << FN_A1_P2 | 1u << FN_A1_P4 | 1u << FN_A1_Q,
   "model bank: only the interleaved-frame kernels (NAM_HIP_KERNEL_A1_IL) run a bank",
   BANK_BLOB_KERNEL_REGION, BANK_MEMBER_SCALARS},
  {"A2 (nam_kq_kernel)", NAM_HIP_KERNEL_A1_MFMA,
   "nam_hip_batch_set_kernel: an A2 bank batch runs nam_kq_kernel / nam_kt_mfma_kernel only (NAM_HIP_KERNEL_AUTO / NAM_HIP_KERNEL_A1_MFMA)",
   1u << FN_KQ | 1u << FN_KT_MFMA,
   "model bank (A2 family): only nam_kq_kernel and nam_kt_mfma_kernel run it; a launch beyond 2^28 frames would take "
   "nam_a1_kernel, which knows no banks: split the launch",
   BANK_BLOB_WHOLE, BANK_MEMBER_SCALARS},
  // (no WaveNet group: pick_kernel is not asked and launch_a1_family not reached; select_kernel answers one of the two functions)
  {"LSTM (nam_lstm_row_kernel / nam_lstm_wide_kernel)", NAM_HIP_KERNEL_AUTO,
   "nam_hip_batch_set_kernel: an LSTM bank batch runs nam_lstm_row_kernel / nam_lstm_wide_kernel only "
   "(NAM_HIP_KERNEL_AUTO); the matrix-core and lanes kernels know no banks",
   1u << FN_LSTM_ROW | 1u << FN_LSTM_WIDE, "", BANK_BLOB_WHOLE, BANK_MEMBER_INIT_STATES},
  // (launch_wr takes the group whatever the stream count: pick_kernel answers the class before the one-model rules)
  {"WN_REG (nam_wn_reg_kernel)", NAM_HIP_KERNEL_WN_REG,
   "nam_hip_batch_set_kernel: a nam_wn_reg_kernel bank batch runs that kernel only (NAM_HIP_KERNEL_AUTO / NAM_HIP_KERNEL_WN_REG)",
   1u << FN_WN_REG, "model bank (nam_wn_reg_kernel family): only nam_wn_reg_kernel runs it", BANK_BLOB_WR, BANK_MEMBER_NOTHING},
};

// A container's submodels as the members of one BANK_A1_IL bank, the largest as member 0 (nam_hip_model::mix_family: MIX_A1): each
// is put to member_refusal and a1_il_difference as a model of its own — its spec, its plan — exactly as nam_hip_bank_create puts
// the members it is given.
std::string container_a1_difference(const nam_hip_model& m)
{
  if (m.spec->arch != ARCH_CONTAINER || m.plans.size() != m.spec->submodels.size())
    return "not a SlimmableContainer with one plan per submodel";
  std::vector<nam_hip_model> sub(m.plans.size());
  for (size_t w = 0; w < sub.size(); w++)
  {
    sub[w].spec = m.spec->submodels[w];
    sub[w].plans.push_back(m.plans[w]);
    sub[w].width_channels.push_back({});
  }
  const size_t order_first = (size_t)m.full_width; // (member 0 first: a refusal of the largest submodel is the first reason)
  for (size_t k = 0; k < sub.size(); k++)
  {
    const size_t w = k == 0 ? order_first : (k <= order_first ? k - 1 : k);
    int fam = BANK_A1_IL;
    const std::string why = member_refusal(sub[w], &fam);
    if (!why.empty())
      return "submodel " + std::to_string(w) + " is " + why;
    FirstDifference diff;
    if (fam != BANK_A1_IL)
      diff.text = std::string("family (") + kBankFamily[fam].name + " vs " + kBankFamily[BANK_A1_IL].name + ")";
    else if (w != order_first)
      kFirstDifference[BANK_A1_IL](diff, sub[order_first], sub[w]);
    if (!diff.text.empty())
      return "submodel " + std::to_string(w) + " differs from the largest submodel in " + diff.text;
  }
  return "";
}

int bank_blob_base(const Plan& p, int family)
{
  return kBankFamily[family].blob_source == BANK_BLOB_KERNEL_REGION ? p.a1.ws_tiles_off : 0;
}
const std::vector<float>& bank_blob(const Plan& p, int family)
{
  return kBankFamily[family].blob_source == BANK_BLOB_WR ? p.wr.blob : p.blob;
}

// The device image of a bank batch's one group (instead of upload_group): every member's kernel region in ONE allocation, the
// per-member scalars (or the per-member initial states: BankFamilyRules::init_states), the per-stream member index.
int upload_bank_group(nam_hip_batch* b, WidthGroup& g)
{
  const nam_hip_bank_data& bank = *b->bank;
  const Plan& p = *g.plan;
  DeviceBuf<float>& d_blobs = kBankFamily[bank.family].blob_source == BANK_BLOB_WR ? g.d_wr_blob : g.d_blob;
  NAM_HIP_CHECK(upload(d_blobs, bank.blobs.data(), bank.blobs.size()));
  if (kBankFamily[bank.family].per_member == BANK_MEMBER_INIT_STATES)
    NAM_HIP_CHECK(upload(g.d_init, bank.init.data(), bank.init.size(), 1));
  else if (kBankFamily[bank.family].per_member == BANK_MEMBER_SCALARS)
  {
    NAM_HIP_CHECK(upload(g.d_a1, &p.a1, 1));
    NAM_HIP_CHECK(upload(g.d_bank_scal, bank.scal.data(), bank.scal.size()));
  }
  NAM_HIP_CHECK(upload(g.d_bank_member, b->stream_member.data(), (size_t)b->n_streams));
  g.bank_stride = bank.blob_stride;
  g.state_stride = p.state_floats;
  return NAM_HIP_OK;
}

// (init_states families) h0 / c0 of their members into `n` streams (`d_map`: which; nullptr = streams 0 .. n - 1), the rest of the state zero.
// On the batch's stream.
int bank_fill_initial_state(nam_hip_batch* b, WidthGroup& g, const int* d_map, int n)
{
  NAM_HIP_CHECK(launch_fill_state_bank(g.d_state.get(), g.state_stride, d_map, n, g.d_init.get(), g.d_bank_member.get(), b->bank->n_init,
                                       g.plan->state_floats, b->stream.get()));
  return NAM_HIP_OK;
}

// nam_hip_batch_set_stream_model behind its argument checks; the order of operations is nam_hip_batch_set_slimmable_size's.
int bank_set_stream_model(nam_hip_batch* b, const int* stream_ids, int n_ids, int member)
{
  std::vector<int> ids;
  if (const int rc = collect_stream_ids(b, stream_ids, n_ids, "nam_hip_batch_set_stream_model", ids))
    return rc;
  std::vector<int> moved;
  for (int s : ids)
    if (b->stream_member[s] != member)
      moved.push_back(s);
  if (moved.empty())
    return NAM_HIP_OK;
  NAM_HIP_CHECK(quiesce(b)); // (a resident launch holds its members' weights since its prologue: it ends here)
  WidthGroup& g = b->groups[b->model->full_width];
  for (int s : moved)
    b->stream_member[s] = member;
  NAM_HIP_CHECK(hipMemcpy(g.d_bank_member.get(), b->stream_member.data(), (size_t)b->n_streams * sizeof(int), hipMemcpyHostToDevice));
  // fresh state of the new member for the streams that moved: Reset (+ prewarm), every other stream untouched.
  // An LSTM's Reset clears nothing (the reference's has nothing to clear: its state is h / c, born from the weight stream), so the
  // moved streams would keep the OLD member's h / c: they get the new member's h0 / c0 here, as a newly created batch's streams do
  return reset_moved_streams(b, g, moved, kBankFamily[b->bank->family].per_member == BANK_MEMBER_INIT_STATES);
}

} // namespace api
} // namespace namhip

extern "C" {

int nam_hip_bank_create(const nam_hip_model* const* models, int n_models, nam_hip_bank** out_bank)
{
  if (!models || !out_bank || n_models <= 0)
    return fail(NAM_HIP_ERR_INVALID_ARGUMENT, "nam_hip_bank_create: bad argument (models, out_bank, n_models >= 1)");
  *out_bank = nullptr;
  for (int i = 0; i < n_models; i++)
    if (!models[i])
      return fail(NAM_HIP_ERR_INVALID_ARGUMENT, "nam_hip_bank_create: member " + std::to_string(i) + " is NULL");
  return guarded([&]() -> int {
    int family = BANK_A1_IL;
    for (int i = 0; i < n_models; i++)
    {
      int fam = BANK_A1_IL;
      const std::string why = member_refusal(*models[i], &fam);
      if (!why.empty())
        return fail(NAM_HIP_ERR_UNSUPPORTED, "nam_hip_bank_create: member " + std::to_string(i) + " is " + why);
      if (i == 0)
        family = fam;
      FirstDifference diff;
      if (fam != family)
        diff.text = std::string("family (") + kBankFamily[fam].name + " vs " + kBankFamily[family].name + "; a bank is of one family)";
      else if (i)
        kFirstDifference[family](diff, *models[0], *models[i]);
      if (!diff.text.empty())
        return fail(NAM_HIP_ERR_UNSUPPORTED,
                    "nam_hip_bank_create: member " + std::to_string(i) + " differs from member 0 in " + diff.text);
    }
    auto data = std::make_shared<nam_hip_bank_data>();
    const nam_hip_model& m0 = *models[0];
    const Plan& p0 = member_plan(m0);
    data->family = family;
    data->proto.spec = member_spec(m0); // (a container member: the submodel's — a bank batch is not slimmable)
    data->proto.plans.push_back(p0);
    data->proto.width_channels.push_back({});
    data->proto.full_width = 0;
    data->n_members = n_models;
    const BankPerMember per_member = kBankFamily[family].per_member;
    const size_t region = bank_blob(p0, family).size() - (size_t)bank_blob_base(p0, family);
    data->blob_stride = (long)((region + 3) / 4 * 4);
    data->blobs.assign((size_t)n_models * (size_t)data->blob_stride, 0.f);
    if (per_member == BANK_MEMBER_INIT_STATES)
    {
      data->n_init = (int)p0.lstm.init_state.size();
      data->init.assign((size_t)n_models * (size_t)data->n_init, 0.f);
    }
    else if (per_member == BANK_MEMBER_SCALARS)
      data->scal.resize((size_t)n_models * 2);
    for (int i = 0; i < n_models; i++) // (stream state blobs name a member by what it computes: stream_state.h)
      data->member_fp.push_back(model_fingerprint(*member_spec(*models[i])));
    data->fingerprint = sstate::fnv1a64(data->member_fp.data(), data->member_fp.size() * sizeof(uint64_t));
    for (int i = 0; i < n_models; i++)
    {
      const Plan& p = member_plan(*models[i]);
      std::memcpy(data->blobs.data() + (size_t)i * (size_t)data->blob_stride, bank_blob(p, family).data() + bank_blob_base(p, family),
                  region * sizeof(float));
      if (per_member == BANK_MEMBER_INIT_STATES)
        std::copy(p.lstm.init_state.begin(), p.lstm.init_state.end(), data->init.begin() + (size_t)i * (size_t)data->n_init);
      if (per_member != BANK_MEMBER_SCALARS)
        continue;
      data->scal[2 * (size_t)i] = p.blob[(size_t)p.a1.head_scale_off];
      // nam_kq_kernel runs ReLU as LeakyReLU with slope 0 (launch_kq does the same for one model)
      data->scal[2 * (size_t)i + 1] = (family == BANK_A2 && p.a1.arr[0].act == ACT_RELU) ? 0.0f : p.a1.arr[0].act_p0;
    }
    nam_hip_bank* bank = new nam_hip_bank();
    bank->data = std::move(data);
    *out_bank = bank;
    return NAM_HIP_OK;
  });
}

void nam_hip_bank_free(nam_hip_bank* bank)
{
  delete bank;
}

int nam_hip_bank_n_models(const nam_hip_bank* bank)
{
  return bank ? bank->data->n_members : NAM_HIP_ERR_INVALID_ARGUMENT;
}

} // extern "C"
