// stream_state.h — the blob nam_hip_batch_get_stream_state writes and nam_hip_batch_set_stream_state reads: its header, how it is
// encoded and validated against a destination, and the index arithmetic of a Linear batch's history ring (whose rows a blob keeps
// oldest frame first, whatever the ring position of the batch it came from). Plain functions of integers and bytes: no HIP header,
// so tests/src/stream_state_check.cpp runs every refusal on the CPU. api_launch.cpp (get_stream_state, set_stream_state) and the
// column kernel next to launch_fill_state (kernel_lstm.hip) are the callers.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

namespace namhip
{
namespace sstate
{
constexpr uint32_t kMagic = 0x5453484eu; // "NHST" in memory order
constexpr uint32_t kVersion = 1;
constexpr int32_t kFamilyFresh = -1; // api_internal.h: STATE_FRESH (freshly zeroed: any layout may follow)

// Everything is fixed-width and naturally aligned: the struct is the byte image (little-endian hosts only, as the device is).
struct Header
{
  uint32_t magic = kMagic;
  uint32_t version = kVersion;
  uint32_t header_bytes = 0; // sizeof(Header): the payload starts there
  int32_t arch = 0; // model_spec.h: Arch of the stream's plan (a container's stream: its submodel's)
  uint64_t model_fp = 0; // the batch's model (config text and weights); a bank: every member's, in order
  uint64_t member_fp = 0; // a bank: the fingerprint of the member the stream runs; else 0
  int32_t member = -1; // a bank: the member index; else -1
  int32_t width = 0; // which of the model's plans the stream runs (a slimmable model's width, a container's submodel; else 0)
  int32_t state_family = kFamilyFresh; // a WaveNet: StateFamily of the stream's group; else kFamilyFresh
  int32_t state_floats = 0; // WaveNet, LSTM: floats of the stream's state row; Linear: 0
  int32_t lin_hist_frames = 0; // Linear: rows of the history ring (LinearPlan::hist_frames of the batch's max_frames); else 0
  int32_t lin_channels = 0; // Linear: the stream's columns (LinearPlan::cols_per_stream); else 0
  // what else the image's layout depends on. nam_wn_reg_kernel's histories: WrPlan::hist_floats and the layer count (the row is
  // [write positions][rings], whatever the launch shape that wrote it); an LSTM: hidden size and layers (every LSTM kernel keeps
  // the row as [layer][h | c][unit]); else 0
  int32_t layout0 = 0, layout1 = 0;
  uint64_t payload_bytes = 0;
  uint64_t payload_sum = 0; // fnv1a64 of the payload
};
static_assert(sizeof(Header) == 80, "the blob's header is a byte image");

inline uint64_t fnv1a64(const void* data, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
  const unsigned char* p = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < n; i++)
    h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

// What one of the destination's plans keeps per stream, and what its group currently holds
struct Geometry
{
  int32_t arch = 0;
  int32_t state_floats = 0, lin_hist_frames = 0, lin_channels = 0, layout0 = 0, layout1 = 0;
  int32_t state_family = kFamilyFresh; // of the destination's group of this width
  uint64_t payload_bytes() const { return 4ull * (arch == 4 /* ARCH_LINEAR */ ? (uint64_t)lin_hist_frames * (uint64_t)lin_channels : (uint64_t)state_floats); }
};
// The destination batch as a blob is compared against it
struct Expect
{
  uint64_t model_fp = 0;
  const uint64_t* member_fp = nullptr; // a bank batch: [n_members]; else nullptr
  int32_t n_members = 0;
  const Geometry* widths = nullptr; // [n_widths]: one per plan of the model
  int32_t n_widths = 0;
};

inline int64_t blob_bytes(const Geometry& g)
{
  return (int64_t)sizeof(Header) + (int64_t)g.payload_bytes();
}

// header + payload into `out` (blob_bytes(g) bytes). `member` < 0: no bank.
inline void encode(void* out, uint64_t model_fp, int member, uint64_t member_fp, int width, const Geometry& g, const void* payload)
{
  Header h;
  h.header_bytes = (uint32_t)sizeof(Header);
  h.arch = g.arch;
  h.model_fp = model_fp;
  h.member_fp = member < 0 ? 0 : member_fp;
  h.member = member < 0 ? -1 : member;
  h.width = width;
  h.state_family = g.state_family;
  h.state_floats = g.state_floats;
  h.lin_hist_frames = g.lin_hist_frames;
  h.lin_channels = g.lin_channels;
  h.layout0 = g.layout0;
  h.layout1 = g.layout1;
  h.payload_bytes = g.payload_bytes();
  h.payload_sum = fnv1a64(payload, (size_t)h.payload_bytes);
  std::memcpy(out, &h, sizeof(h));
  if (h.payload_bytes)
    std::memcpy(static_cast<char*>(out) + sizeof(h), payload, (size_t)h.payload_bytes);
}

// "" when the blob fits the destination (then `out` is its header and the payload is buf + sizeof(Header)), else the refusal:
// it names the field. Reads nothing beyond `size` bytes.
inline std::string validate(const void* buf, int64_t size, const Expect& e, Header& out)
{
  if (!buf || size < (int64_t)sizeof(Header))
    return "size: the blob is shorter than its header (truncated)";
  Header h;
  std::memcpy(&h, buf, sizeof(h));
  if (h.magic != kMagic)
    return "magic: not a stream state blob";
  if (h.version != kVersion)
    return "version: format " + std::to_string(h.version) + ", this library reads " + std::to_string(kVersion);
  if (h.header_bytes != sizeof(Header))
    return "header_bytes: corrupted header";
  if (h.payload_bytes > (uint64_t)INT64_MAX - sizeof(Header) || (int64_t)(sizeof(Header) + h.payload_bytes) != size)
    return "size: " + std::to_string(size) + " bytes given, the header announces " + std::to_string(sizeof(Header)) + " + "
           + std::to_string(h.payload_bytes) + " (truncated or corrupted)";
  if (h.model_fp != e.model_fp)
    return "model_fp: the blob was taken from a stream of another model";
  if (e.member_fp)
  {
    if (h.member < 0 || h.member >= e.n_members)
      return "member: index " + std::to_string(h.member) + " outside the bank";
    if (h.member_fp != e.member_fp[h.member])
      return "member_fp: the blob's member is another model than the bank's member " + std::to_string(h.member);
  }
  else if (h.member != -1 || h.member_fp != 0)
    return "member: the blob names a bank member, the batch has no bank";
  if (h.width < 0 || h.width >= e.n_widths)
    return "width: index " + std::to_string(h.width) + " outside the model's plans";
  const Geometry& g = e.widths[h.width];
  if (h.arch != g.arch)
    return "arch: the blob's architecture is not the stream's";
  if (h.state_floats != g.state_floats)
    return "state_floats: " + std::to_string(h.state_floats) + " in the blob, " + std::to_string(g.state_floats) + " in the batch";
  if (h.lin_hist_frames != g.lin_hist_frames)
    return "lin_hist_frames: " + std::to_string(h.lin_hist_frames) + " rows in the blob, " + std::to_string(g.lin_hist_frames)
           + " in the batch (another max_frames class)";
  if (h.lin_channels != g.lin_channels)
    return "lin_channels: " + std::to_string(h.lin_channels) + " in the blob, " + std::to_string(g.lin_channels) + " in the batch";
  if (h.layout0 != g.layout0 || h.layout1 != g.layout1)
    return "layout: the state row is laid out differently";
  if (h.payload_bytes != g.payload_bytes())
    return "payload_bytes: " + std::to_string(h.payload_bytes) + " in the blob, the geometry needs " + std::to_string(g.payload_bytes());
  if (h.state_family < kFamilyFresh || h.state_family > 2)
    return "state_family: corrupted header";
  if (h.state_family != kFamilyFresh && g.state_family != kFamilyFresh && h.state_family != g.state_family)
    return "state_family: the state was written in another kernel family's layout; reset first";
  if (fnv1a64(static_cast<const char*>(buf) + sizeof(Header), (size_t)h.payload_bytes) != h.payload_sum)
    return "payload_sum: the payload does not match its checksum (corrupted)";
  out = h;
  return std::string();
}

// ---- a Linear batch's history ring [hist_frames][columns]: `pos` is the row the NEXT frame goes to, so the oldest row ----
// Canonical row j (0 = the oldest frame, hist_frames - 1 = the newest) of a ring at position `pos` (0 <= pos < hist_frames).
// constexpr: the device code asks the same function.
constexpr int ring_row(int pos, int j, int hist_frames)
{
  return pos + j >= hist_frames ? pos + j - hist_frames : pos + j;
}

} // namespace sstate
} // namespace namhip
