// csrc/stream_state.h on the CPU (tests/test_stream_state_format.py builds this with AddressSanitizer + UBSan; no device, nothing
// preloaded): a stream state blob's round trip, every refusal with the field it names, truncation at every header boundary (the
// blob sits at the END of a heap block of exactly its length, so a read past it is a sanitizer report), a flipped byte, and the
// Linear ring's row arithmetic for every pair of positions against a plain modular restatement.
#include <cstddef>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "stream_state.h"

using namespace namhip::sstate;

static int failures = 0;

#define CHECK(cond)                                                             \
  do                                                                            \
  {                                                                             \
    if (!(cond))                                                                \
    {                                                                           \
      std::printf("stream_state_check: line %d: %s\n", __LINE__, #cond);        \
      failures++;                                                               \
    }                                                                           \
  } while (0)

// validate() on a heap copy of exactly `n` bytes
static std::string check_copy(const std::vector<unsigned char>& blob, size_t n, const Expect& e, Header& h)
{
  std::unique_ptr<unsigned char[]> exact(new unsigned char[n ? n : 1]);
  std::memcpy(exact.get(), blob.data(), n);
  return validate(exact.get(), (int64_t)n, e, h);
}
static bool names(const std::string& why, const char* field)
{
  return why.rfind(std::string(field) + ":", 0) == 0;
}

static Geometry wavenet_geometry(int family)
{
  Geometry g;
  g.arch = 1;
  g.state_floats = 192;
  g.layout0 = 128;
  g.layout1 = 3;
  g.state_family = family;
  return g;
}

static std::vector<unsigned char> make_blob(uint64_t model_fp, int member, uint64_t member_fp, int width, const Geometry& g)
{
  std::vector<float> payload((size_t)g.payload_bytes() / 4);
  for (size_t i = 0; i < payload.size(); i++)
    payload[i] = 0.25f * (float)i - 3.0f;
  std::vector<unsigned char> blob((size_t)blob_bytes(g));
  encode(blob.data(), model_fp, member, member_fp, width, g, payload.data());
  return blob;
}

static void round_trip_and_refusals()
{
  const uint64_t fp = 0x1234567890abcdefull;
  const Geometry src = wavenet_geometry(1);
  const std::vector<unsigned char> blob = make_blob(fp, -1, 0, 0, src);
  CHECK(blob.size() == sizeof(Header) + 192 * 4);

  Geometry dst[2] = {wavenet_geometry(kFamilyFresh), wavenet_geometry(kFamilyFresh)};
  dst[1].state_floats = 64;
  Expect e;
  e.model_fp = fp;
  e.widths = dst;
  e.n_widths = 2;
  Header h;
  // the round trip: a fresh destination takes any family; the same family fits; the header comes back as written
  CHECK(check_copy(blob, blob.size(), e, h).empty());
  CHECK(h.magic == kMagic && h.version == kVersion && h.arch == 1 && h.model_fp == fp && h.member == -1 && h.width == 0 && h.state_family == 1
        && h.state_floats == 192 && h.layout0 == 128 && h.layout1 == 3 && h.payload_bytes == 192 * 4);
  {
    const float* p = reinterpret_cast<const float*>(blob.data() + sizeof(Header));
    CHECK(p[0] == -3.0f && p[191] == 0.25f * 191 - 3.0f);
  }
  dst[0].state_family = 1;
  CHECK(check_copy(blob, blob.size(), e, h).empty());
  // another non-fresh family: the existing "reset first"
  dst[0].state_family = 0;
  {
    const std::string why = check_copy(blob, blob.size(), e, h);
    CHECK(names(why, "state_family") && why.find("reset first") != std::string::npos);
  }
  // a STATE_FRESH blob fits anywhere
  {
    const std::vector<unsigned char> fresh = make_blob(fp, -1, 0, 0, wavenet_geometry(kFamilyFresh));
    for (int fam = -1; fam <= 2; fam++)
    {
      dst[0].state_family = fam;
      CHECK(check_copy(fresh, fresh.size(), e, h).empty());
    }
  }
  dst[0].state_family = kFamilyFresh;
  // another model
  {
    Expect o = e;
    o.model_fp = fp + 1;
    CHECK(names(check_copy(blob, blob.size(), o, h), "model_fp"));
  }
  // another geometry, field by field
  {
    Geometry g2[2] = {dst[0], dst[1]};
    Expect o = e;
    o.widths = g2;
    g2[0] = dst[0];
    g2[0].state_floats = 256;
    CHECK(names(check_copy(blob, blob.size(), o, h), "state_floats"));
    g2[0] = dst[0];
    g2[0].layout0 = 64;
    CHECK(names(check_copy(blob, blob.size(), o, h), "layout"));
    g2[0] = dst[0];
    g2[0].arch = 2;
    CHECK(names(check_copy(blob, blob.size(), o, h), "arch"));
    o.n_widths = 0;
    CHECK(names(check_copy(blob, blob.size(), o, h), "width"));
  }
  // a blob of the second width lands there
  {
    Geometry narrow = dst[1];
    narrow.state_family = 2;
    const std::vector<unsigned char> b1 = make_blob(fp, -1, 0, 1, narrow);
    CHECK(check_copy(b1, b1.size(), e, h).empty() && h.width == 1 && h.state_floats == 64);
  }
  // truncation: every length from nothing to one byte short, the header's field boundaries among them
  for (size_t n = 0; n < blob.size(); n++)
    CHECK(names(check_copy(blob, n, e, h), "size"));
  // ... and a longer buffer than the header announces
  {
    std::vector<unsigned char> longer = blob;
    longer.push_back(0);
    CHECK(names(check_copy(longer, longer.size(), e, h), "size"));
  }
  // a flipped payload byte (first, middle, last), a flipped bit of every header byte
  for (size_t at : {sizeof(Header), sizeof(Header) + 333, blob.size() - 1})
  {
    std::vector<unsigned char> bad = blob;
    bad[at] ^= 0x10;
    CHECK(names(check_copy(bad, bad.size(), e, h), "payload_sum"));
  }
  for (size_t at = 0; at < sizeof(Header); at++)
  {
    std::vector<unsigned char> bad = blob;
    bad[at] ^= 0x01;
    const std::string why = check_copy(bad, bad.size(), e, h);
    // (state_family 1 -> 0 against a fresh destination is another VALID header: the one flip no check can see)
    const bool family_byte = at == offsetof(Header, state_family);
    CHECK(family_byte ? why.empty() : !why.empty());
  }
  {
    std::vector<unsigned char> bad = blob;
    bad[0] ^= 0xff;
    CHECK(names(check_copy(bad, bad.size(), e, h), "magic"));
    bad = blob;
    bad[4] = 2;
    CHECK(names(check_copy(bad, bad.size(), e, h), "version"));
    bad = blob;
    bad[8] = 81;
    CHECK(names(check_copy(bad, bad.size(), e, h), "header_bytes"));
  }
  CHECK(names(validate(nullptr, 100, e, h), "size"));
}

static void banks()
{
  const uint64_t bank_fp = 77, members[3] = {11, 22, 33};
  Geometry lstm;
  lstm.arch = 2;
  lstm.state_floats = 64;
  lstm.layout0 = 18;
  lstm.layout1 = 2;
  Expect e;
  e.model_fp = bank_fp;
  e.member_fp = members;
  e.n_members = 3;
  e.widths = &lstm;
  e.n_widths = 1;
  Header h;
  const std::vector<unsigned char> blob = make_blob(bank_fp, 2, 33, 0, lstm);
  CHECK(check_copy(blob, blob.size(), e, h).empty() && h.member == 2 && h.member_fp == 33 && h.state_family == kFamilyFresh);
  // another member fingerprint; a member outside the bank; a bank blob on a one-model batch and the reverse
  const std::vector<unsigned char> other = make_blob(bank_fp, 2, 34, 0, lstm);
  CHECK(names(check_copy(other, other.size(), e, h), "member_fp"));
  const std::vector<unsigned char> outside = make_blob(bank_fp, 3, 33, 0, lstm);
  CHECK(names(check_copy(outside, outside.size(), e, h), "member"));
  Expect one = e;
  one.member_fp = nullptr;
  one.n_members = 0;
  CHECK(names(check_copy(blob, blob.size(), one, h), "member"));
  const std::vector<unsigned char> plain = make_blob(bank_fp, -1, 0, 0, lstm);
  CHECK(names(check_copy(plain, plain.size(), e, h), "member"));
  CHECK(check_copy(plain, plain.size(), one, h).empty());
}

static void linear_geometry()
{
  Geometry lin;
  lin.arch = 4;
  lin.lin_hist_frames = 640;
  lin.lin_channels = 2;
  CHECK(lin.payload_bytes() == 640u * 2u * 4u);
  Expect e;
  e.model_fp = 5;
  e.widths = &lin;
  e.n_widths = 1;
  Header h;
  const std::vector<unsigned char> blob = make_blob(5, -1, 0, 0, lin);
  CHECK(check_copy(blob, blob.size(), e, h).empty() && h.lin_hist_frames == 640 && h.lin_channels == 2 && h.state_floats == 0);
  // another max_frames class: another ring length
  Geometry longer = lin;
  longer.lin_hist_frames = 1152;
  Expect o = e;
  o.widths = &longer;
  {
    const std::string why = check_copy(blob, blob.size(), o, h);
    CHECK(names(why, "lin_hist_frames") && why.find("max_frames") != std::string::npos);
  }
  Geometry mono = lin;
  mono.lin_channels = 1;
  o.widths = &mono;
  CHECK(names(check_copy(blob, blob.size(), o, h), "lin_channels"));
}

// The rotation of a ring of L rows. The source ring holds frame number f (0 = the oldest) in row (sp + f) mod L. Gathered at
// every source position the rows come out oldest first; scattered at every destination position dp, frame f sits in row
// (dp + f) mod L, so the row the next frame goes to, dp, holds the oldest. Every PAIR (sp, dp): where a source row lands, against
// the plain modular form (every frame of the short ring; every 97th, the first and the last of the long one).
static void rotation(int L)
{
  std::vector<int> src((size_t)L), rows((size_t)L), dst((size_t)L);
  for (int sp = 0; sp < L; sp++)
  {
    for (int f = 0; f < L; f++)
      src[(size_t)((sp + f) % L)] = f;
    bool canonical = true;
    for (int j = 0; j < L; j++)
    {
      const int r = ring_row(sp, j, L);
      canonical = canonical && r >= 0 && r < L && src[(size_t)r] == j;
    }
    CHECK(canonical);
  }
  for (int j = 0; j < L; j++)
    rows[(size_t)j] = j;
  for (int dp = 0; dp < L; dp++)
  {
    dst.assign((size_t)L, -1);
    for (int j = 0; j < L; j++)
    {
      const int r = ring_row(dp, j, L);
      CHECK(r >= 0 && r < L);
      dst[(size_t)r] = rows[(size_t)j];
    }
    bool ok = dst[(size_t)dp] == 0 && dst[(size_t)((dp + L - 1) % L)] == L - 1;
    for (int f = 0; f < L; f++)
      ok = ok && dst[(size_t)((dp + f) % L)] == f;
    CHECK(ok);
  }
  const int step = L > 64 ? 97 : 1;
  for (int sp = 0; sp < L; sp++)
    for (int dp = 0; dp < L; dp++)
    {
      // frame j is gathered from source row ring_row(sp, j) and scattered to destination row ring_row(dp, j)
      auto moved_ok = [&](int j) {
        const int from = ring_row(sp, j, L), to = ring_row(dp, j, L);
        return from == (sp + j) % L && to == ((from - sp + L) % L + dp) % L;
      };
      // the oldest row goes where the destination writes next, the newest just before it
      bool ok = moved_ok(0) && moved_ok(L - 1) && ring_row(dp, 0, L) == dp && ring_row(dp, L - 1, L) == (dp + L - 1) % L;
      for (int j = 0; j < L; j += step)
        ok = ok && moved_ok(j);
      if (!ok)
      {
        std::printf("stream_state_check: rotation L=%d sp=%d dp=%d\n", L, sp, dp);
        failures++;
        return;
      }
    }
}

int main()
{
  round_trip_and_refusals();
  banks();
  linear_geometry();
  rotation(7);
  rotation(896);
  if (failures)
  {
    std::printf("stream_state_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("stream_state_check: ok\n");
  return 0;
}
