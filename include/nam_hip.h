/*
 * nam_hip.h — C ABI of the MI355X-native NAM inference core (libnam_hip.so).
 *
 * Drop-in boundary for ONE hot path of sdatkinson/NeuralAmpModelerCore: running many independent
 * audio streams through one .nam model (`nam::get_dsp(path)` + `nam::DSP::process(in, out, n)`).
 * The reference exposes that path as a C++ class API, not a C ABI; the entry points below are what
 * a binding for that path needs, each citing the reference interface it replaces
 * (file:line relative to the reference tree). The C++ adapter in cpp/NAM/ re-creates the
 * reference's `nam::DSP` / `nam::get_dsp` signatures on top of this ABI.
 *
 * Conventions
 *   - every function returns NAM_HIP_OK (0) or a negative error code; the message of the last
 *     error on the calling thread is available from nam_hip_last_error(). No C++ exception ever
 *     crosses this boundary (the reference throws at load time: NAM/nam_file.h:11,
 *     NAM/get_dsp.cpp:116-121, NAM/wavenet/model.cpp:671-682, and asserts at run time
 *     NAM/wavenet/model.cpp:824).
 *   - audio is planar: buffer[stream][channel][frame]; the *_f32 / *_f64 entry points take HOST
 *     pointers (they copy to and from the GPU), the *_device entry point takes DEVICE pointers and
 *     an optional hipStream_t and does not synchronise.
 *   - a `nam_hip_model` is immutable host data (parsed file + device plans); a `nam_hip_batch`
 *     owns the GPU memory (weights, per-stream history) for N streams of one model on one device
 *     and must be used from one host thread at a time, like a reference `nam::DSP` instance.
 *     A `nam_hip_bank` is an immutable set of models one batch runs side by side (nam_hip_batch_create_bank).
 */
#ifndef NAM_HIP_H
#define NAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
  #define NAM_HIP_API __attribute__((visibility("default")))
#else
  #define NAM_HIP_API
#endif

#define NAM_HIP_OK 0
#define NAM_HIP_ERR_INVALID_ARGUMENT (-1)
#define NAM_HIP_ERR_FILE (-2) /* nam::NamFileValidationError — NAM/nam_file.cpp:9-40 */
#define NAM_HIP_ERR_MODEL (-3) /* std::runtime_error at load: bad version / config / weight count */
#define NAM_HIP_ERR_UNSUPPORTED (-4) /* valid .nam the device path cannot run (e.g. ConvNet; a Linear model beyond the device limits below) */
#define NAM_HIP_ERR_DEVICE (-5) /* HIP runtime error */
#define NAM_HIP_ERR_TOO_MANY_FRAMES (-6) /* num_frames > max_frames (assert in NAM/wavenet/model.cpp:824) */

#define NAM_HIP_ARCH_WAVENET 1
#define NAM_HIP_ARCH_LSTM 2
#define NAM_HIP_ARCH_CONTAINER 3 /* SlimmableContainer: submodels selected by nam_hip_batch_set_slimmable_size */
#define NAM_HIP_ARCH_LINEAR 4 /* an impulse response (NAM/linear.cpp): see "Linear models" below */

/* ---- Linear models (nam::Linear, NAM/linear.cpp, NAM/linear.h; history: nam::Buffer, NAM/dsp.cpp:203-305) ----
 * Function: for channels ch < min(in_channels, out_channels): y[ch][n] = bias + sum_{k < receptive_field} weights[k] * x[ch][n - k],
 *   history zero at the start; one impulse response for every channel, no mixing (linear.cpp:177-189); output channels
 *   >= min(in, out) are 0, not the bias (linear.cpp:191-195). Exactly receptive_field (+ 1 with "bias": the last one) weights,
 *   else "Params vector does not match expected size based on architecture parameters" (linear.cpp:68-72).
 *   GetPrewarmSamples() is 0 (the DSP base, dsp.h:153): Reset with prewarm processes nothing.
 * "implementation" ("auto" | "direct" / "legacy" / "old" | "fft" / "partitioned_fft" / "partitioned-fft", any letter case;
 *   anything else fails with "Unsupported Linear implementation: <as given>", linear.cpp:280-293) selects between the reference's
 *   two CPU engines, which compute the same function with different roundings. It selects NOTHING on the device: it is validated,
 *   kept in NAM_HIP_FIELD_CONFIG_JSON, and otherwise ignored — one device engine computes every Linear model.
 * Device limits: receptive_field <= 65,536 (1.4 s at 48 kHz), in_channels and out_channels <= 16; beyond either the load fails
 *   with NAM_HIP_ERR_UNSUPPORTED and a message naming the limit. receptive_field < 1 or a channel count < 1: NAM_HIP_ERR_MODEL.
 * Reset: nam_hip_batch_reset ZEROES a Linear batch's input history — the state of a freshly constructed reference model. A
 *   deliberate choice, because the reference has no single behaviour to mirror: its direct engine keeps the input history across
 *   Reset (Buffer::Reset / _set_receptive_field are not called from Linear::Reset, linear.cpp:83-97), its FFT engine rebuilds the
 *   partition state but keeps the direct-tap buffer (linear.cpp:109-165). (Compare the LSTM note at nam_hip_batch_reset.)
 * Kernels: nam_linear_kernel (what nam_hip_batch_kernel_name* report, for every launch length) between an append and a reduce
 *   kernel per launch piece: 64 frames x 32 columns of output are one fp32 matrix product of the impulse response's Toeplitz matrix
 *   with the input history, on v_mfma_f32_32x32x2_f32 — exact float32, fused multiply-adds; the taps are cut into K-splits whose
 *   partial sums are added in a fixed order: the same call sequence gives the same bits, run to run and at any stream count.
 *   How a stream is cut into calls changes results only through the order of summation (as under NAM_HIP_KERNEL_AUTO elsewhere).
 *   nam_hip_model_info::state_bytes_per_stream is the history a batch with max_frames <= 512 keeps per stream (a longer max_frames,
 *   up to 4,096, adds the difference): (taps rounded up to whole K-splits + one launch piece) frames x min(in, out) channels.
 * A Linear batch supports create / destroy / reset, process_f32 / _f64 / _device (any length, frame_stride), render_f32,
 *   submit / wait, synchronize, n_streams, kernel_name*. nam_hip_batch_set_persistent returns 0 (a model without recurrence has
 *   nothing to keep resident; calls launch as usual); nam_hip_batch_set_kernel accepts NAM_HIP_KERNEL_AUTO, anything else is
 *   NAM_HIP_ERR_UNSUPPORTED; set_slimmable_size returns what it returns for any non-slimmable model.
 *   NAM_HIP_ERR_UNSUPPORTED too: a Linear model as a member of a bank (nam_hip_bank_create), as a submodel of a SlimmableContainer
 *   that also holds submodels of another architecture ("SlimmableContainer: submodel i is a Linear model ...", naming the first),
 *   or as a WaveNet's condition_dsp.
 * A SlimmableContainer whose submodels are ALL Linear, each 1-in / 1-out (one impulse response at several lengths; a submodel with
 *   more channels fails with the container's mono message), loads: architecture NAM_HIP_ARCH_CONTAINER, is_slimmable 1,
 *   prewarm_samples 0, nam_hip_model_slimmable_breakpoints = the max_values but the last. Its batch keeps ONE input ring for all
 *   streams, as long as the longest submodel needs (state_bytes_per_stream: one column of it), and every stream runs the submodel
 *   nam_hip_batch_set_slimmable_size chose for it (ModelSpec::container_index, container.cpp:85-97; a new batch: the last one) —
 *   per-stream impulse responses in one launch: nam_linear_pairs_kernel (what kernel_name* report) between the append kernel and a
 *   reduce kernel, three launches per piece however many sizes are in use.
 *   Contract: a stream on submodel w produces, BIT FOR BIT, what a one-model Linear batch of w produces for the same input (same
 *   K-splits, taps oldest first as one chain of fused multiply-adds, partial sums in split order, the bias last), for finite input,
 *   counted from the stream's last reset or size change — at any stream count and whatever the other streams run.
 *   set_slimmable_size: a stream that changes submodel starts from a freshly reset one (its column of the ring becomes zero); a
 *   stream already on that submodel, the ring position and every stream not named are untouched. nam_hip_batch_reset zeroes the
 *   ring and keeps the sizes; restart_streams zeroes the streams' columns and keeps their sizes. A stream state blob records the
 *   container and the stream's submodel (its width); the payload is the stream's column, oldest frame first; set_stream_state moves
 *   the stream to the blob's submodel without the reset. Everything a Linear batch supports works, with the same answers from
 *   set_persistent (0) and set_kernel (NAM_HIP_KERNEL_AUTO only). As a bank member the container stays refused. */

/* kernel selection for nam_hip_batch_set_kernel */
#define NAM_HIP_KERNEL_AUTO 0
#define NAM_HIP_KERNEL_GENERIC 1 /* op-program interpreter (every WaveNet feature) */
#define NAM_HIP_KERNEL_A1 2 /* register-resident VALU kernel for the plain A1 family (1 wave per stream) */
#define NAM_HIP_KERNEL_A1_MFMA 3 /* fp32-MFMA kernels for the A1 family: kernel size 3 everywhere -> wave-specialised kernel
                                    (4 compute + 4 mover waves per stream); a single layer array with other kernel
                                    sizes (A2) -> K-tap kernel (4 waves per stream). Narrower submodels of a container
                                    that neither can run use NAM_HIP_KERNEL_A1 */

#define NAM_HIP_KERNEL_A1_IL 4 /* interleaved-frame fp32-MFMA kernels of the official WaveNet sizes (two arrays of ten layers,
                                  kernel size 3, dilations 1..512; 16/8, 12/8, 8/4 channels): compute wave w owns frames 4j + w,
                                  so dilations 4..32 are DPP row shifts inside the wave and dilations >= 64 the lane's own ring
                                  rows; launches of more than one buffer run the pipelined forms. Any other topology falls
                                  back to NAM_HIP_KERNEL_A1_MFMA */
#define NAM_HIP_KERNEL_WN_REG 5 /* register-resident WaveNet kernel for narrow, feature-rich models (FiLMs, gating, grouped
                                   1x1s, head1x1, a nested condition_dsp — example_models/wavenet_a2_max.nam): one wavefront
                                   per stream, lane = frame, a layer = one unrolled function per instantiated shape; every
                                   conv reaches at most 64 frames back. AUTO picks it when no A1 kernel takes the model;
                                   falls back like AUTO when the model's shapes are not instantiated */

typedef struct nam_hip_model nam_hip_model;
typedef struct nam_hip_batch nam_hip_batch;
typedef struct nam_hip_bank nam_hip_bank;

/* What nam::DSP's getters report — NAM/dsp.h:100-149,153, NAM/slimmable.h:23-29. */
typedef struct nam_hip_model_info
{
  int32_t architecture; /* NAM_HIP_ARCH_* */
  int32_t in_channels; /* DSP::NumInputChannels  dsp.h:104 */
  int32_t out_channels; /* DSP::NumOutputChannels dsp.h:108 */
  int32_t prewarm_samples; /* DSP::GetPrewarmSamples dsp.h:153 (WaveNet: model.cpp:653-658; LSTM: lstm.cpp:127-134) */
  double expected_sample_rate; /* DSP::GetExpectedSampleRate dsp.h:100; -1.0 when the file has none */
  int32_t has_loudness; /* DSP::HasLoudness dsp.h:137 */
  int32_t has_input_level; /* DSP::HasInputLevel */
  int32_t has_output_level; /* DSP::HasOutputLevel */
  int32_t is_slimmable; /* dynamic_cast<SlimmableModel*> succeeds — slimmable.h:13 */
  double loudness; /* DSP::GetLoudness dsp.h:125 */
  double input_level; /* DSP::GetInputLevel dsp.h:116 */
  double output_level; /* DSP::GetOutputLevel dsp.h:133 */
  int64_t num_weights;
  int32_t fast_tanh; /* load-time switch replacing the global Activation::enable_fast_tanh (activations.cpp:168) */
  int32_t has_a1_kernel; /* bit 0: the A1 VALU kernel can run this model; bit 1: one of the A1 MFMA kernels can; bits 2 and 3
                            (always equal since 0.2.1): the interleaved-frame MFMA kernels can — the official WaveNet sizes, job tables compiled in;
                            bit 4: nam_wn_reg_kernel can; bit 5: the model asked for nam_wn_reg_kernel compiled for its own layer
                            shapes and that compile was not available here (no compiler / sources / private cache directory:
                            a line on stderr and NAM_HIP_FIELD_DESCRIPTION say why) — it runs, on a slower form */
  int64_t state_bytes_per_stream; /* HBM history per stream */
  char version[32]; /* .nam "version" */
} nam_hip_model_info;

/* Message of the last failure on this thread ("" if none). */
NAM_HIP_API const char* nam_hip_last_error(void);

/* ---- loading: nam::get_dsp(path / json) — NAM/get_dsp.h:85-116, NAM/get_dsp.cpp:156-273 ----
 * fast_tanh != 0 mirrors calling nam::activations::Activation::enable_fast_tanh() before get_dsp
 * (tools/benchmodel.cpp:69-73): "Tanh" layers use the rational approximation (activations.h:91-98)
 * and LSTM cells use fast_sigmoid / fast_tanh (lstm.cpp:48-58). */
NAM_HIP_API int nam_hip_model_load(const char* nam_path, int fast_tanh, nam_hip_model** out_model);
NAM_HIP_API int nam_hip_model_load_json(const char* json_text, int fast_tanh, nam_hip_model** out_model);

/* Everything the reference keeps in process-globals around get_dsp, as explicit load options:
 *   fast_tanh  Activation::enable_fast_tanh()                       NAM/activations.cpp:168-177
 *   luts       Activation::enable_lut(function_name, min, max, n)   NAM/activations.cpp:189-212: "Tanh", "Sigmoid" or
 *              "SiLU" layers of the model use FastLUTActivation (NAM/activations.h:371-422: clamp, linear
 *              interpolation in a table of n points built with the host's libm). A table wins over fast_tanh, as it
 *              does when enable_lut is called after enable_fast_tanh. Any other name fails with the reference's message.
 * Exactly one of nam_path / json_text must be non-NULL; options == NULL means all defaults. */
typedef struct nam_hip_lut
{
  const char* function_name;
  float min_x, max_x;
  int32_t n_points;
} nam_hip_lut;
typedef struct nam_hip_load_options
{
  int32_t fast_tanh;
  int32_t n_luts;
  const nam_hip_lut* luts;
  /* != 0: the caller has already run the version gate — verify_config_version with its own registered
   * IVersionSupportChecker objects (NAM/get_dsp.h:19-25,60, get_dsp.cpp:92-128), which can only WIDEN what the core
   * checker accepts — so the library's built-in gate (0.5.0 <= version, minor <= 0.7) is skipped. */
  int32_t version_checked_by_caller;
  /* sizeof(nam_hip_load_options) as the CALLER compiled it (NAM_HIP_LOAD_OPTIONS_INIT sets it). The library reads a field behind
   * the first 16 bytes (fast_tanh, n_luts, luts) only if struct_size says the caller's struct holds it.
   * ABI NOTE (library 0.2.0): this field took the slot of 0.1's `reserved` (that header was 24 bytes: fast_tanh, n_luts, luts,
   * version_checked_by_caller, reserved = 0). A binary built against the 0.1 header therefore passes struct_size = 0 and its
   * version_checked_by_caller is IGNORED — the safe direction: the built-in version gate stays on, a widened file is rejected
   * with the reference's message rather than loaded unchecked. Such callers must be rebuilt against this header
   * (nam_hip_version() reports "0.2.x"); 0 also covers callers that zero-fill, so garbage behind a short struct can never
   * switch the gate off. */
  int32_t struct_size;
} nam_hip_load_options;
#define NAM_HIP_LOAD_OPTIONS_INIT {0, 0, 0, 0, (int32_t)sizeof(nam_hip_load_options)}
/* With version_checked_by_caller the caller's checkers have seen the TOP-LEVEL document only: nested documents (a WaveNet's
 * condition_dsp, a container's submodels) still pass the library's built-in gate, where the reference consults its registry on
 * every get_dsp call (NAM/get_dsp.cpp:92-128). A caller that widens support for nested files must check them itself. */
NAM_HIP_API int nam_hip_model_load_ex(const char* nam_path, const char* json_text, const nam_hip_load_options* options,
                                      nam_hip_model** out_model);
NAM_HIP_API void nam_hip_model_free(nam_hip_model* model);
NAM_HIP_API int nam_hip_model_get_info(const nam_hip_model* model, nam_hip_model_info* info);

/* ---- nam::dspData (NAM/dsp.h:348-357) across the boundary: get_dsp(dspData&) NAM/get_dsp.h:91, get_dsp(path, dspData&
 * returnedConfig) :101, get_dsp(json, dspData& returnedConfig) :109, get_sample_rate_from_nam_file :121 ----
 * nam_hip_model_load_parts builds a model from the fields of a dspData: version, architecture, the "config" value as JSON
 * text, the "metadata" value as JSON text (NULL or "null": none), the weights, expected_sample_rate (-1.0: unknown).
 * It runs verify_config_version + the architecture's config parser + weight binding (get_dsp.cpp:232-261), and fails
 * the way those do. */
NAM_HIP_API int nam_hip_model_load_parts(const char* version, const char* architecture, const char* config_json,
                                         const char* metadata_json, const float* weights, int64_t n_weights,
                                         double expected_sample_rate, const nam_hip_load_options* options,
                                         nam_hip_model** out_model);
/* The dspData of a loaded model (populate_dsp_data, get_dsp.cpp:141-154). String fields: */
#define NAM_HIP_FIELD_VERSION 0
#define NAM_HIP_FIELD_ARCHITECTURE 1
#define NAM_HIP_FIELD_CONFIG_JSON 2 /* the "config" value, compact JSON text */
#define NAM_HIP_FIELD_METADATA_JSON 3 /* the "metadata" value ("null" when the file has none) */
#define NAM_HIP_FIELD_DESCRIPTION 4 /* not dspData: one line about the device plans (which kernels take the model, and why                                        nam_wn_reg_kernel does not when it does not) */
/* Copies up to capacity - 1 bytes + NUL into buf (buf may be NULL); returns the full length (>= 0) or an error code. */
NAM_HIP_API int64_t nam_hip_model_get_string(const nam_hip_model* model, int field, char* buf, int64_t capacity);
/* Copies up to `capacity` weights (out may be NULL); returns their number. A SlimmableContainer has none of its own. */
NAM_HIP_API int64_t nam_hip_model_get_weights(const nam_hip_model* model, float* out, int64_t capacity);
/* get_sample_rate_from_nam_file (NAM/get_dsp.h:121, get_dsp.cpp:275-281) on a .nam document given as a path or as text
 * (exactly one non-NULL): "sample_rate" if present, else -1.0. */
NAM_HIP_API int nam_hip_sample_rate_from_nam(const char* nam_path, const char* json_text, double* out_sample_rate);

/* SlimmableModel::GetSlimmableSizeBreakpoints — NAM/slimmable.h:29, NAM/wavenet/slimmable.cpp:108-121.
 * Writes up to `capacity` values, returns the number available (>= 0) or an error code. */
NAM_HIP_API int nam_hip_model_slimmable_breakpoints(const nam_hip_model* model, double* out, int capacity);

/* ---- batches: N independent streams of one model on one GPU ----
 * Replaces N instances of nam::DSP. `max_frames` plays the role of maxBufferSize in
 * DSP::Reset(sampleRate, maxBufferSize) (NAM/dsp.cpp:130-140): the largest n_frames a process call
 * may pass, and the chunk size used for prewarming (NAM/dsp.cpp:86-100). History starts zeroed
 * (Conv1D::SetMaxBufferSize, NAM/conv1d.cpp:128-149); LSTM state starts from the file's h0/c0
 * (NAM/lstm.cpp:24-28). `device` is the HIP device ordinal. */
NAM_HIP_API int nam_hip_batch_create(const nam_hip_model* model, int device, int n_streams, int max_frames,
                         nam_hip_batch** out_batch);
NAM_HIP_API void nam_hip_batch_destroy(nam_hip_batch* batch);

/* ---- model banks: one batch whose streams each run their own model ("captures") ----
 * A host that serves captures runs one architecture with many weight sets. A bank is an immutable set of loaded models that
 * ONE batch runs side by side — one launch, one session, one ticket queue — each stream bound to one member.
 * nam_hip_bank_create is host-only (no device call). A bank is of ONE family, decided by member 0, and accepts a set when every
 * member plans onto the same instantiation of that family's kernels with the same blob and state layout:
 *  - the interleaved-frame kernels: the official WaveNet topology (two arrays of ten layers, kernel size 3, dilations 1 .. 512)
 *    at 16 / 8 channels — the lite 12 / 6 and feather 8 / 4 sizes are zero-padded to it at plan time —, all members Tanh or all
 *    Fasttanh (so: loaded with the same fast_tanh), no lookup tables;
 *  - the A2 family (nam_kq_kernel, nam_kt_mfma_kernel): WaveNets of the A2 topology (one array of 8 channels, 23 layers with
 *    kernel sizes 6 / 15, a 16-tap head rechannel) whose activation nam_kq_kernel is compiled for — exactly the models whose
 *    one-model batch is session-eligible on that kernel. All members share the activation TYPE (all LeakyReLU, all ReLU, all
 *    Tanh or all Fasttanh); the LeakyReLU negative slope (<= 1) is per member, like head_scale. A SlimmableContainer (how A2
 *    captures ship: A2.nam holds A2-Lite and A2-Full) may be a member when its LARGEST submodel qualifies; the member IS that
 *    submodel — the one a batch of the container runs while no size has been set. No lookup tables.
 *  - the LSTM family (nam_lstm_row_kernel, nam_lstm_wide_kernel): LSTMs of ONE shape — the same layer count (1 or 2), input
 *    size (1 or 2), hidden size (<= 32) and output channels —, loaded with the same fast_tanh, from files of one sample rate
 *    (the prewarm is half a second of it). A member's initial state (h0 / c0, part of an LSTM's weight stream) is its own.
 *    Larger cells run on kernels whose streams share one wavefront's weights: they are refused.
 *  - the nam_wn_reg_kernel family: non-slimmable WaveNets whose one-model batch runs on nam_wn_reg_kernel under AUTO — the
 *    official nano size (4 -> 2 channels), FiLM / gated models, a nested condition_dsp, a post-stack head, narrow plain
 *    stacks — of ONE program: the same topology (arrays, channels, kernel sizes, dilations, FiLM sets, activation types),
 *    loaded with the same fast_tanh. Weights, head_scale and a nested condition's head scale are per member (a per-model code
 *    object has the scales compiled in; a bank launch runs member 0's and reads each member's own from its weights).
 *    (A plain A2-Lite-shaped WaveNet is of this family too; a SlimmableContainer never is: it stands for its largest submodel.)
 * The plans are compared field by field; the first difference — a member of another family, or of another kind: another
 * topology or activation type, a lookup-table activation, a slimmable model — is refused with NAM_HIP_ERR_UNSUPPORTED and a message naming the member index and the field. n_models <= 0
 * or a NULL member: NAM_HIP_ERR_INVALID_ARGUMENT. A bank of one model is legal. The bank copies what it needs: the models may
 * be freed right after, and the bank may be freed while batches created from it live. */
NAM_HIP_API int nam_hip_bank_create(const nam_hip_model* const* models, int n_models, nam_hip_bank** out_bank);
NAM_HIP_API void nam_hip_bank_free(nam_hip_bank* bank);
/* Number of members (>= 1), or NAM_HIP_ERR_INVALID_ARGUMENT for a NULL bank. */
NAM_HIP_API int nam_hip_bank_n_models(const nam_hip_bank* bank);
/* nam_hip_batch_create for a bank: stream s runs member stream_model[s] (NULL: every stream member 0; an index outside
 * [0, n_models) is NAM_HIP_ERR_INVALID_ARGUMENT). The result is an ordinary batch: reset, process_*, render, set_persistent,
 * flush, submit / wait, synchronize, kernel_name* and n_streams work as for one model; set_slimmable_size returns what it
 * returns for a non-slimmable model. The members' weights live in one device allocation [member][blob]; a workgroup resolves
 * its stream's member once, in the kernel's prologue. Kernels of a bank of the official topology: the NAM_HIP_KERNEL_A1_IL
 * family for every launch shape — nam_a1_q_kernel in sessions and launches of several buffers, nam_a1_p4_kernel for short
 * bursts and short blocking calls, nam_a1_p2_kernel for a lone buffer (where a one-model batch under AUTO runs
 * nam_a1_mfma_kernel, which knows no banks); nam_hip_batch_set_kernel accepts NAM_HIP_KERNEL_AUTO and NAM_HIP_KERNEL_A1_IL,
 * anything else is NAM_HIP_ERR_UNSUPPORTED. Kernels of an A2 bank: what a one-model A2 batch runs under AUTO — nam_kq_kernel
 * in sessions and launches of several buffers (renders, the prewarm of Reset), nam_kt_mfma_kernel for a lone buffer and for
 * everything under NAM_HIP_MAX_STAGES=1; nam_hip_batch_set_kernel accepts NAM_HIP_KERNEL_AUTO and NAM_HIP_KERNEL_A1_MFMA,
 * anything else is NAM_HIP_ERR_UNSUPPORTED; one launch of more than 2^28 frames (which a one-model batch hands to
 * nam_a1_kernel) is NAM_HIP_ERR_UNSUPPORTED: split it. Kernels of an LSTM bank: nam_lstm_row_kernel (hidden <= 4) or
 * nam_lstm_wide_kernel for every launch shape and in sessions; nam_hip_batch_set_kernel accepts NAM_HIP_KERNEL_AUTO only
 * (the matrix-core and lanes kernels know no banks), anything else is NAM_HIP_ERR_UNSUPPORTED. Kernels of a nam_wn_reg_kernel
 * bank: that kernel for every launch shape, in sessions, and at EVERY stream count (a one-model batch of a plain narrow model
 * beyond 8 x workgroups-per-CU x CUs streams flips to nam_a1_kernel; the bank does not, it then has no session);
 * nam_hip_batch_set_kernel accepts NAM_HIP_KERNEL_AUTO and NAM_HIP_KERNEL_WN_REG, anything else is NAM_HIP_ERR_UNSUPPORTED.
 * Reset with prewarm runs the silence through every stream with its own member's weights (no cached image: it depends on the
 * weights); the state equals, bit for bit, what a one-model batch of that member holds after the same Reset. */
NAM_HIP_API int nam_hip_batch_create_bank(const nam_hip_bank* bank, int device, int n_streams, int max_frames,
                                          const int* stream_model, nam_hip_batch** out_batch);
/* Binds the listed streams (NULL: all) to `member`, following nam_hip_batch_set_slimmable_size's contract: a running session's
 * launch ends first (the kernels load weights in their prologue), the streams that change member start from a freshly reset
 * (and, if the batch was last reset with prewarm, prewarmed) state of the new member — an LSTM member's own h0 / c0, then the
 * prewarm: what a newly created one-model batch of that member holds after the same Reset —; every other stream's state and output
 * are untouched; a stream already bound to `member` is left alone. A stream or member out of range — or a batch that was not
 * created from a bank — is NAM_HIP_ERR_INVALID_ARGUMENT and changes nothing. */
NAM_HIP_API int nam_hip_batch_set_stream_model(nam_hip_batch* batch, const int* stream_ids, int n_ids, int member);
/* The member `stream` is bound to (0 for every stream of a one-model batch), or NAM_HIP_ERR_INVALID_ARGUMENT. */
NAM_HIP_API int nam_hip_batch_get_stream_model(const nam_hip_batch* batch, int stream);

/* DSP::Reset (NAM/dsp.cpp:130-140): WaveNet history is zeroed; if `prewarm` != 0 the model then
 * processes ceil(prewarm_samples / max_frames) * max_frames frames of silence (DSP::prewarm,
 * NAM/dsp.cpp:67-101). LSTM recurrent state is NOT re-initialised by Reset in the reference
 * (NAM/lstm.cpp has no SetMaxBufferSize override); this call mirrors that: LSTM batches only prewarm. */
NAM_HIP_API int nam_hip_batch_reset(nam_hip_batch* batch, int prewarm);

/* ---- stream slots: restart one stream of a live batch, save and restore it ----
 * A batch is N slots that players come to and leave. These four calls are blocking, take host memory and belong to the
 * non-real-time side, like Reset. Like nam_hip_batch_set_slimmable_size each one first quiesces the batch: a running session's
 * launch ends and hands the state back, tickets in flight complete and stay available to wait, a remembered caller stream is
 * waited for. None of them changes the state or the output of a stream it does not name.
 *
 * nam_hip_batch_restart_streams: the listed streams (stream_ids == NULL: all; duplicates are allowed) take, bit for bit, the
 * state a NEWLY CREATED batch of the same model or bank and max_frames (any stream count) holds after
 * nam_hip_batch_reset(batch, prewarm). A WaveNet stream: zeroed history, then the prewarm (or the cached prewarmed image). An
 * LSTM stream: its h0 / c0 from the weight stream (a bank: its member's) FIRST, then the prewarm — unlike nam_hip_batch_reset,
 * which mirrors the reference and leaves h / c alone, so that a recycled slot does not start from the previous player's
 * recurrent state. A Linear stream: its own columns of the batch's history ring become zero (the ring position and every other
 * stream's columns stay). A slimmable stream keeps its width, a bank stream its member. An id out of range is
 * NAM_HIP_ERR_INVALID_ARGUMENT and changes nothing. */
NAM_HIP_API int nam_hip_batch_restart_streams(nam_hip_batch* batch, const int* stream_ids, int n_ids, int prewarm);
/* One stream's state as an opaque, self-describing blob: get on one batch, set on the same or on another one (another stream
 * count, another GPU, another process with the same library version): a rewind, a checkpoint, a move. From the next call on the
 * destination stream produces exactly the bits the source stream would have produced (under the same kernel: kernels of
 * different launch classes differ by ~1e-7 by design).
 * The blob records a magic and format version, the architecture, a 64-bit fingerprint of the model (config text and weights),
 * for a bank the member index and that member's fingerprint, for a slimmable model the width, for a WaveNet the layout its
 * state is in (the op program's rings / the zero-padded A1 rings / nam_wn_reg_kernel's histories / freshly zeroed), the payload
 * length and what it depends on, and a checksum of the payload. Payload: the stream's state row (WaveNet: write positions and
 * rings; LSTM: h / c per layer), or for a Linear stream its columns of the history ring, oldest frame first — independent of
 * the source batch's ring position.
 * nam_hip_batch_stream_state_size: the bytes get writes for `stream` now (it depends on the stream's width), or an error code.
 * nam_hip_batch_get_stream_state: writes the blob to buf and its size to *out_size (out_size may be NULL). A capacity that is
 * too small is NAM_HIP_ERR_INVALID_ARGUMENT with the needed size in *out_size; nothing is written to buf.
 * nam_hip_batch_set_stream_state: validates everything before it touches the batch, then moves the stream to the blob's width
 * (as nam_hip_batch_set_slimmable_size moves it, without the reset), binds it to the blob's member (nam_hip_batch_get_stream_model
 * reports it from then on) and writes the state (a Linear stream's rows rotated to the destination's ring position). Refused with
 * NAM_HIP_ERR_INVALID_ARGUMENT, a message that names the field, and nothing changed: a blob of another model or whose member is
 * another model than the bank's; another payload geometry (a Linear batch of another max_frames class); a truncated or
 * corrupted blob; a blob whose WaveNet layout differs from what the destination's streams of that width hold ("reset first":
 * a freshly zeroed blob fits anywhere, and freshly zeroed streams take the blob's layout).
 * A2 containers at mixed sizes in persistent mode (nam_hip_batch_set_persistent): an A2-Lite stream's blob is ALWAYS in
 * nam_wn_reg_kernel's layout, whichever way the stream currently lives — get copies a zero-padded stream's rings out into that
 * layout (the padded channels are dropped), set copies them in (the padded channels become zero) —, so the blob format, its size
 * and where it may go (an all-Lite batch, a mixed one, persistent or not) do not depend on the batch it came from.
 * nam_hip_batch_restart_streams works on either kind of stream of such a batch.
 * Containers of the official WaveNet topology's sizes (standard, lite, feather) at mixed sizes in persistent mode: a lite or
 * feather stream's blob is its own submodel's zero-padded rings, the layout it has in either residence — get copies the stream's
 * row out of the standard submodel's rows first, set writes it into the stream's own row and the row moves back in —, so here
 * too the blob's format, size and acceptable destinations are the same whether the batch is resident or not. */
NAM_HIP_API int64_t nam_hip_batch_stream_state_size(const nam_hip_batch* batch, int stream);
NAM_HIP_API int nam_hip_batch_get_stream_state(nam_hip_batch* batch, int stream, void* buf, int64_t capacity, int64_t* out_size);
NAM_HIP_API int nam_hip_batch_set_stream_state(nam_hip_batch* batch, int stream, const void* buf, int64_t size);

/* SlimmableModel::SetSlimmableSize(val) for a subset of the streams (NAM/slimmable.h:23,
 * NAM/wavenet/slimmable.cpp:420-431,527-530): the listed streams switch to the sub-model of width
 * ratio_to_channels(ratio) and start from a freshly reset (and, if the batch was last reset with
 * prewarm, prewarmed) state, as the reference's rebuilt model does. stream_ids == NULL selects all.
 * Every stream the call does not name keeps its state — also where the call mixes or un-mixes an A2 container's batch in
 * persistent mode and those streams change the kernel they run on (nam_hip_batch_set_persistent): their histories are copied
 * into the other kernel's layout, float for float. The same holds for a container of the official WaveNet topology's sizes
 * (standard, lite, feather): there the rows of the streams the call does not name are copied whole, bit for bit. */
NAM_HIP_API int nam_hip_batch_set_slimmable_size(nam_hip_batch* batch, const int* stream_ids, int n_ids, double ratio);

/* DSP::process(NAM_SAMPLE** input, NAM_SAMPLE** output, int num_frames) — NAM/dsp.h:97,
 * NAM/wavenet/model.cpp:822-910, NAM/lstm.cpp:103-125 — for all streams of the batch at once.
 * in  : [n_streams][in_channels ][n_frames]   out : [n_streams][out_channels][n_frames]  (host memory)
 * n_frames must be <= max_frames. Blocks until the output is in `out`. The _f64 form is for callers
 * built with NAM_SAMPLE = double (NAM/dsp.h:18-22); the model itself computes in float32
 * (cast-in NAM/wavenet/model.cpp:817, cast-out :896). */
NAM_HIP_API int nam_hip_batch_process_f32(nam_hip_batch* batch, const float* in, float* out, int n_frames);
NAM_HIP_API int nam_hip_batch_process_f64(nam_hip_batch* batch, const double* in, double* out, int n_frames);

/* Same computation on buffers already resident in HBM (offline re-amping / batch render):
 * d_in / d_out are DEVICE pointers laid out [n_streams][channels][frame_stride]; frames
 * [0, n_frames) of every row are consumed / produced. n_frames may be any length (the kernel walks
 * it in 64-frame blocks, exactly as tools/render.cpp:146-197 walks a file in 64-frame buffers).
 * Enqueues on `hip_stream` (a hipStream_t, NULL = the batch's own stream) and returns without
 * synchronising. */
NAM_HIP_API int nam_hip_batch_process_device(nam_hip_batch* batch, const float* d_in, float* d_out, int n_frames,
                                 int64_t frame_stride, void* hip_stream);

/* Offline render ("re-amp") of whole signals: stream s reads n_frames[s] frames from the planar host buffer
 * in[s] ([in_channels][n_frames[s]]) and writes out[s] ([out_channels][n_frames[s]]). Signals may have different
 * lengths (shorter ones are zero-padded on the device; their tails are discarded). Equivalent to feeding every
 * stream through process() in 64-frame buffers the way tools/render.cpp:129-191 does — for a given kernel the results do
 * not depend on the buffer partition (under NAM_HIP_KERNEL_AUTO a launch of four or more blocks may run another kernel of
 * the same family than a one-block launch: same state, sums associated differently, ~1e-7) — but runs as one resident
 * launch over device-resident audio. Blocking.
 * Replaces the block loop of the reference's render tool (tools/render.cpp:163-197). */
NAM_HIP_API int nam_hip_batch_render_f32(nam_hip_batch* batch, const float* const* in, float* const* out,
                                         const int64_t* n_frames);

/* Persistent block mode (opt-in; nam_a1_q_kernel / nam_a1_p4_kernel, nam_kq_kernel, nam_wn_reg_kernel — mixed slimmable widths included — and
 * the small LSTM kernels): instead of one kernel launch per nam_hip_batch_process_device call, a SESSION launch consumes
 * every call of up to 2,048 frames — of ANY length on nam_wn_reg_kernel and the LSTM kernels (n_frames / 64 whole commands and
 * one partial command of 1 .. 63 frames: 32- and 48-frame hosts, 120 / 240 / 480-frame network packets stay on the resident
 * launch), of a multiple of 64 frames on nam_a1_q_kernel / nam_a1_p4_kernel / nam_kq_kernel (n_frames / 64 commands; their
 * pipelines hand fixed sub-blocks from stage to stage) — a command is a 64-bit word in a
 * device-memory ring, stored by the host itself when the call's stream is idle, else by hipStreamWriteValue64 on that
 * stream, so it is ordered behind whatever produced the input there — for as long as the next command is already there
 * when a buffer is finished, and leaves as soon as the ring is empty (a device-wide synchronize never waits for a
 * session; the next call starts the launch again). A launch that serves HOST buffers — tickets, or blocking *_f32 / *_f64 calls
 * that come back to back (the previous one returned less than 50 us ago) — stores one completion word per command instead, so the
 * call waits for its own buffer only, and lingers for the next one for a bounded time (200 us: NAM_HIP_TICKET_LINGER_US,
 * NAM_HIP_BLOCKING_LINGER_US; 0 = never; a device-wide synchronize then waits for the linger at most): on every session kernel,
 * the pipeline kernels and nam_wn_reg_kernel / the LSTM kernels alike. What a launch per buffer pays on top of the computation (dispatch,
 * cold prologue, state in and out: 4-12 us) is paid once per burst.
 * Consecutive calls must address the same resident window (d_in / d_out of the first call plus a common frame offset,
 * same frame_stride, offsets of any alignment; device memory or host-mapped memory); anything else — another window, Reset,
 * SetSlimmableSize, set_kernel, a render, destroy, and on the three pipeline kernels a length that is no multiple of 64 (it runs
 * as a plain launch; the next whole buffer starts a session again) — ends the session first (the launch writes the streams'
 * state back), transparently. A session that has carried partial commands is renumbered (one flush and session start) every 2^25
 * commands — 9.3 hours of 48-frame calls at 48 kHz — instead of every 2^30 (csrc/session_command.h). The blocking *_f32 / *_f64 entry points stay inside the session (host-mapped staging).
 * Outputs are NOT ordered on the caller's stream: call nam_hip_batch_flush (or nam_hip_batch_synchronize, or use the
 * blocking *_f32 / *_f64 entry points, which do it) before consuming them.
 * Eligible: one width group on nam_a1_q_kernel / nam_a1_p4_kernel / nam_kq_kernel up to 8 streams per CU (beyond one per CU the workgroups
 * take turns on the chip); every group on nam_wn_reg_kernel up to 8 x min(4, 160 KB / LDS image) streams per CU (in turns too); small LSTMs.
 * A SlimmableContainer of the A2 family (A2.nam: A2-Lite and A2-Full, submodels that differ in channel count only) whose streams
 * are at MIXED sizes is eligible as ONE group on nam_kq_kernel, up to 8 streams per CU: while the mode is on, the narrower streams
 * run zero-padded copies of their submodel (exact: zero weights and biases on the padded rows) next to the Full ones — one
 * resident launch, one command ring; tickets, the blocking calls' linger, per-command completion and flush as on an all-Full
 * batch, a length that is no multiple of 64 frames as on an all-Full batch too (one plain launch of nam_kt_mfma_kernel over every
 * stream). All-Lite batches keep nam_wn_reg_kernel, all-Full ones nam_kq_kernel. The control calls that mix or un-mix a batch
 * (this one, nam_hip_batch_set_slimmable_size, nam_hip_batch_set_stream_state, nam_hip_batch_reset, nam_hip_batch_set_kernel) move
 * the state of the narrow streams they do NOT name between the two kernels' layouts — a copy of the same histories at the same
 * ring positions, so those streams go on undisturbed; no process call ever does. Outside the mode such a batch launches per size,
 * as ever. nam_hip_batch_kernel_name* answer nam_kq_kernel / nam_kt_mfma_kernel for such a batch whatever the sizes' shares: every
 * stream runs them.
 * The same rule for the official WaveNet topology (standard 16 / 8, lite 12 / 6, feather 8 / 4 channels): a SlimmableContainer
 * qualifies when EVERY submodel plans onto the padded 16 / 8 layout with a nam_a1_q_kernel plan — each one a model a bank of the
 * interleaved-frame family would take, all with one activation and one fast_tanh, none differing from the largest in a field
 * nam_hip_bank_create compares (NAM_HIP_FIELD_DESCRIPTION says "a1_mixed_session=1", or "=0" and the first difference). Its
 * streams at MIXED sizes are ONE group on the BANK forms of nam_a1_q_kernel / nam_a1_p4_kernel, up to 8 streams per CU, member =
 * the stream's submodel: one resident launch, one command ring; tickets, linger, per-command completion, flush and the
 * short-burst switch to nam_a1_p4_kernel as on an all-standard batch; a length that is no multiple of 64 frames ends the session
 * and runs one plain launch over every stream (nam_a1_p2_kernel, as a bank batch of that family). While the mode is on every
 * stream's rings live in the standard submodel's state rows: a lite or feather stream's own rows have that layout already, so the
 * control calls listed above copy whole rows (nam_state_rows_copy_kernel), bit for bit, and only there. nam_hip_batch_set_kernel:
 * NAM_HIP_KERNEL_AUTO and NAM_HIP_KERNEL_A1_IL keep such a batch in the mode, any other choice takes it out. A batch whose
 * streams are all at one size runs what it always ran. Not covered: a nano tier (4 / 2 channels: outside nam_a1_q_kernel's plan
 * family, it lives on nam_wn_reg_kernel; one such submodel and the container does not qualify), model banks of containers,
 * slimmable WaveNets of the slice method, Linear models.
 * Returns 1 if the batch will use the mode, 0 if it is not eligible (the calls then launch as usual).
 * Allocation: this call and nam_hip_batch_reset — the non-real-time side of the reference's contract (NAM/dsp.h:163) — allocate
 * everything a session needs (command ring, completion words, its stream and events, the host windows of the blocking entry points);
 * no process / submit / wait / flush call allocates.
 * First-buffer latency: a session of the official 16 / 8 WaveNet topology whose caller has flushed after at most four buffers three
 * times in a row starts its next launches as nam_a1_p4_kernel (four waves per layer: the first buffer of a launch is through in a
 * few microseconds) instead of nam_a1_q_kernel (sixteen one-wave stages: higher throughput once buffers overlap), and goes back after
 * a longer burst; both work on the same stream state. nam_hip_batch_kernel_name reports what the next launch starts as. */
NAM_HIP_API int nam_hip_batch_set_persistent(nam_hip_batch* batch, int enable);
/* Blocks until every buffer submitted so far has been rendered and is visible (hip_stream: the stream the process
 * calls were issued on; NULL = the batch's own). No-op outside persistent mode. */
NAM_HIP_API int nam_hip_batch_flush(nam_hip_batch* batch, void* hip_stream);

/* DSP::process (NAM/dsp.h:97) for callers that keep buffers IN FLIGHT — a server feeding many streams from a network
 * thread, an offline renderer reading a file ahead: submit copies `in` ([n_streams][in_channels][n_frames], host memory;
 * the caller may reuse it at once), starts the work and returns a ticket; wait blocks until that buffer's output is
 * there and copies it to `out` ([n_streams][out_channels][the submit's n_frames]; NULL: completed and discarded). Up to
 * NAM_HIP_PIPE_SLOTS tickets may be in flight (the next submit fails with NAM_HIP_ERR_INVALID_ARGUMENT until the oldest
 * has been waited for); buffers are rendered in submit order, a ticket is waited for once, in any order.
 * In persistent mode (nam_hip_batch_set_persistent) buffers are commands of the session — of any length on nam_wn_reg_kernel and
 * the LSTM kernels, of a multiple of 64 frames on the pipeline kernels (another length there is rendered at once by plain
 * launches and handed out by the wait) —, the
 * input written through the PCIe window, the output stored to host memory by the resident launch itself — every session
 * kernel (nam_a1_q_kernel, nam_kq_kernel, nam_wn_reg_kernel in all its forms, nam_lstm_row_kernel, nam_lstm_wide_kernel)
 * publishes every command, so a wait returns when the ticket's own last command is through, while the launch runs on with the
 * buffers behind it. (The pipeline of nam_a1_q_kernel holds five to six
 * 64-frame buffers at a time: keep at least eight in flight at that size, four at 256 frames.) Outside persistent mode: pinned staging, copies and the
 * launch enqueued on the batch's stream, an event behind them. Control calls (Reset, SetSlimmableSize, set_kernel,
 * synchronize) complete the tickets in flight first; their outputs stay available to wait. A ticket session's launch
 * looks for the next buffer for 200 us before it leaves (NAM_HIP_TICKET_LINGER_US; it holds its CUs meanwhile) when all its
 * workgroups are on the chip at once; a batch of more streams than that runs its session in turns, publishes every command all
 * the same and leaves whenever the ring is empty. The blocking process calls may be mixed in (tickets in flight complete first). */
#define NAM_HIP_PIPE_SLOTS 16
NAM_HIP_API int nam_hip_batch_submit_f32(nam_hip_batch* batch, const float* in, int n_frames, int64_t* out_ticket);
NAM_HIP_API int nam_hip_batch_wait_f32(nam_hip_batch* batch, int64_t ticket, float* out);
/* The same for callers built with NAM_SAMPLE = double (NAM/dsp.h:18-22): cast in as NAM/wavenet/model.cpp:817, out as :896. */
NAM_HIP_API int nam_hip_batch_submit_f64(nam_hip_batch* batch, const double* in, int n_frames, int64_t* out_ticket);
NAM_HIP_API int nam_hip_batch_wait_f64(nam_hip_batch* batch, int64_t ticket, double* out);

/* Wait for everything enqueued on the batch's own stream (and on the last caller-supplied one). Ends a persistent
 * session: afterwards nothing of the batch is running on the device (a device-wide hipDeviceSynchronize would
 * otherwise wait for the resident launch to expire). */
NAM_HIP_API int nam_hip_batch_synchronize(nam_hip_batch* batch);

/* Choose the kernel (NAM_HIP_KERNEL_*); AUTO picks the fastest kernel the model allows
 * (A1_MFMA > A1 > GENERIC). */
NAM_HIP_API int nam_hip_batch_set_kernel(nam_hip_batch* batch, int kernel);
NAM_HIP_API int nam_hip_batch_get_kernel(const nam_hip_batch* batch);
NAM_HIP_API int nam_hip_batch_n_streams(const nam_hip_batch* batch);
/* Name of the __global__ function the batch's largest stream group currently runs ("nam_a1_mfma_kernel",
 * "nam_kt_mfma_kernel", "nam_a1_kernel", "nam_generic_kernel", "nam_lstm_mfma_reg_kernel", ...): the name
 * rocprofv3 --kernel-trace reports (without template arguments), so measurements can be attributed to the right kernel. */
NAM_HIP_API const char* nam_hip_batch_kernel_name(const nam_hip_batch* batch);
/* The same question for a launch of n_frames (nam_hip_batch_kernel_name answers it for one 64-frame buffer): under
 * NAM_HIP_KERNEL_AUTO a launch that walks four or more blocks — an offline render, the prewarm of Reset — runs the
 * interleaved-frame kernel where a one-block launch runs the wave-specialised one. */
NAM_HIP_API const char* nam_hip_batch_kernel_name_for(const nam_hip_batch* batch, int n_frames);

/* Developer tool, not part of the drop-in surface: runs n_frames of silence through the MFMA kernel's profiling
 * instantiation; out_stamps (96 x 8 int64) receives, per wavefront w of workgroup 0 (row w): barrier cycles, total
 * cycles, and for compute waves five per-job segment sums (tools/mfma_barrier_profile.py). */
NAM_HIP_API int nam_hip_batch_debug_timeline(nam_hip_batch* batch, int n_frames, long long* out_stamps);

/* Number of HIP devices this process can see (what `device` of nam_hip_batch_create indexes; honours
 * HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES). For hosts that spread batches over the GPUs of a node (cpp/NAM/multi_device.h). */
NAM_HIP_API int nam_hip_device_count(int* out_count);

/* The built-in version gate (CoreVersionSupportChecker, NAM/get_dsp.cpp:18-39): 0 = not supported, 1 = partially (newer
 * patch level than the latest fully supported file version), 2 = fully. */
NAM_HIP_API int nam_hip_version_support(const char* nam_file_version);

/* Library identification: "nam_hip <version> gfx950". */
NAM_HIP_API const char* nam_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* NAM_HIP_H */
