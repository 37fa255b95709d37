// csrc/session_command.h on the CPU (tests/test_session_command.py builds this plainly and with AddressSanitizer + UBSan; no
// device, nothing preloaded): the session's command word — round trips for every frame count at the offsets that matter, a whole
// command bit for bit the word `(tag << 32) | offset`, the split of a call into commands, the tag limit of partial commands and
// what it means for the rebase mark.
#include <cstdio>
#include <initializer_list>

#include "session_command.h"

using namespace namhip::session;

static int failures = 0;

#define CHECK(cond)                                                             \
  do                                                                            \
  {                                                                             \
    if (!(cond))                                                                \
    {                                                                           \
      std::printf("session_command_check: line %d: %s\n", __LINE__, #cond);     \
      failures++;                                                               \
    }                                                                           \
  } while (0)

// compile-time use, as the kernels and the host make of it
static_assert(encode(1u, 0u, 64) == (1ull << 32), "the first whole command");
static_assert(decode(encode(7u, 48u, 17)).n == 17 && decode(encode(7u, 48u, 17)).tag == 7u && decode(encode(7u, 48u, 17)).off == 48u, "a partial command");
static_assert(command_count(480) == 8 && command_frames(480, 7) == 32, "a 10 ms packet at 48 kHz");
static_assert(kPartialRebaseAt == (1u << 25) && kPartialTagMax == kPartialRebaseAt - 1u, "the header's claim");

static void round_trips()
{
  const unsigned offs[] = {0u, 1u, 63u, 64u, 0x1fff0000u, kOffMax};
  // tags: the first, around the partial limit, and (whole commands only) around the old numbering's ends
  const unsigned partial_tags[] = {1u, 2u, 1023u, 1024u, 1025u, kPartialTagMax - 1u, kPartialTagMax};
  const unsigned whole_tags[] = {1u, 2u, 1024u, kPartialTagMax, kPartialTagMax + 1u, 0x3fffffffu, 0x40000000u, kWholeTagMax};
  for (unsigned off : offs)
  {
    for (int n = 1; n <= 64; n++)
      for (unsigned tag : partial_tags)
      {
        const unsigned long long w = encode(tag, off, n);
        const Command c = decode(w);
        CHECK(c.tag == tag);
        CHECK(c.off == off);
        CHECK(c.n == n);
        CHECK(tag_of_hi((unsigned)(w >> 32)) == tag && frames_of_hi((unsigned)(w >> 32)) == n);
        CHECK((unsigned)w == off); // the offset keeps the whole low half, whatever the count
        if (n < 64)
        {
          CHECK((w & kPartialBit) != 0);
          CHECK(((w >> kCountShift) & 63u) == (unsigned)n);
          // never mistaken for the whole command of any tag a workgroup could stand at: bit 63 is clear in all of those
          CHECK((unsigned)(w >> 32) > kWholeTagMax);
        }
      }
    for (unsigned tag : whole_tags)
    {
      const unsigned long long w = encode(tag, off, 64);
      CHECK(w == (((unsigned long long)tag << 32) | off)); // the parent's word, bit for bit
      CHECK((w & kPartialBit) == 0);
      CHECK(tag >= (1u << kPartialTagBits) || ((w >> kCountShift) & 63u) == 0u); // the count field of a whole command is 0 (where the tag leaves it alone)
      const Command c = decode(w);
      CHECK(c.tag == tag && c.off == off && c.n == 64);
    }
  }
  // a stale or empty ring slot is nobody's command
  CHECK(decode(0ull).tag == 0u);
  CHECK(decode(~0ull).tag == kPartialTagMax && decode(~0ull).n == 63); // (the "leave" word is never read as a command; its decode is at least defined)
}

struct Piece
{
  int off, n;
};
static void split(int n_frames, std::initializer_list<Piece> want)
{
  CHECK(command_count(n_frames) == (int)want.size());
  CHECK(has_partial(n_frames) == (n_frames % 64 != 0));
  int i = 0, total = 0;
  for (const Piece& p : want)
  {
    CHECK(command_offset(i) == p.off);
    CHECK(command_frames(n_frames, i) == p.n);
    CHECK(command_offset(i) == total); // contiguous, in order
    total += command_frames(n_frames, i);
    CHECK(i + 1 == (int)want.size() || command_frames(n_frames, i) == 64); // only the last one may be partial
    i++;
  }
  CHECK(total == n_frames);
}

static void splits()
{
  split(1, {{0, 1}});
  split(63, {{0, 63}});
  split(64, {{0, 64}});
  split(65, {{0, 64}, {64, 1}});
  split(120, {{0, 64}, {64, 56}});
  split(480, {{0, 64}, {64, 64}, {128, 64}, {192, 64}, {256, 64}, {320, 64}, {384, 64}, {448, 32}});
  CHECK(command_count(2047) == 32 && command_frames(2047, 31) == 63 && command_offset(31) == 1984);
  CHECK(command_count(2048) == 32 && command_frames(2048, 31) == 64 && !has_partial(2048));
  for (int n : {2047, 2048})
  {
    int total = 0;
    for (int i = 0; i < command_count(n); i++)
    {
      CHECK(command_offset(i) == total);
      CHECK(command_frames(n, i) >= 1 && command_frames(n, i) <= 64);
      total += command_frames(n, i);
    }
    CHECK(total == n);
  }
  CHECK(command_count(0) == 0 && !has_partial(0));
}

static void limits()
{
  const unsigned rebase_at = 0x40000000u; // PersistSession's default mark
  // whole-buffer callers: the mark is where it was, whatever the count
  for (int n : {64, 128, 2048})
  {
    CHECK(rebase_mark(n, rebase_at) == rebase_at);
    const unsigned k = (unsigned)(n / 64);
    CHECK(call_fits(rebase_at - k - 1u, n, rebase_at));
    CHECK(!call_fits(rebase_at - k, n, rebase_at)); // the parent's `seq + n / 64 >= rebase_at`
    CHECK(call_fits(kPartialRebaseAt + 5u, n, rebase_at)); // beyond the partial limit whole commands go on
  }
  // calls with a partial command: every tag of the call at most kPartialTagMax
  for (int n : {1, 17, 63, 65, 120, 480, 2047})
  {
    const unsigned k = (unsigned)command_count(n);
    CHECK(rebase_mark(n, rebase_at) == kPartialRebaseAt);
    const unsigned last_ok = kPartialRebaseAt - k - 1u; // commands submitted before the call
    CHECK(call_fits(last_ok, n, rebase_at));
    CHECK(last_ok + k <= kPartialTagMax); // the call's last tag (its partial command's)
    CHECK(decode(encode(last_ok + k, 5u, command_frames(n, (int)k - 1))).tag == last_ok + k);
    CHECK(!call_fits(last_ok + 1u, n, rebase_at));
    CHECK(rebase_mark(n, 1000u) == 1000u && !call_fits(1000u - k, n, 1000u)); // a lower mark of the session's own (NAM_HIP_PERSIST_REBASE_AT) holds
  }
  // what the header says this costs: 2^25 commands of 48 frames at 48 kHz are 9.3 hours, of 32 frames 6.2 hours
  const double h48 = (double)kPartialRebaseAt * 48.0 / 48000.0 / 3600.0, h32 = (double)kPartialRebaseAt * 32.0 / 48000.0 / 3600.0;
  const double h120 = (double)kPartialRebaseAt / 2.0 * 120.0 / 48000.0 / 3600.0;
  CHECK(h48 > 9.3 && h48 < 9.4);
  CHECK(h32 > 6.2 && h32 < 6.3);
  CHECK(h120 > 11.6 && h120 < 11.7);
  CHECK(kWindowMaxOff == 0x1fff0000l && (unsigned long long)kWindowMaxOff <= kOffMax);
}

int main()
{
  round_trips();
  splits();
  limits();
  if (failures)
  {
    std::printf("session_command_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("session_command_check: ok\n");
  return 0;
}
