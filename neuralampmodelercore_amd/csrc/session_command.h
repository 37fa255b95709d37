// session_command.h — the word a persistent session consumes per buffer (api_session.cpp stores it, persist_wave.h and the
// pipeline kernels read it), the split of a call into such words, and the limits the encoding sets: plain constexpr functions of
// integers. No HIP header, so tests/src/session_command_check.cpp asks them on the CPU; host and device include the same text.
//
// A WHOLE command (64 frames) is the word it has always been:
//     bits 63..32  tag = the command's number in the session, counted from 1 (bit 63 clear: tags stay below 2^31, bit 31 of
//                  the completion words is the "left" flag)
//     bits 31..0   frame offset of the buffer in the session's window
// nam_a1_q_kernel, nam_a1_p4_kernel, nam_a1_p2_kernel and nam_kq_kernel read exactly that and never see anything else.
//
// A PARTIAL command (1 .. 63 frames; nam_wn_reg_kernel, nam_lstm_row_kernel, nam_lstm_wide_kernel) sets bit 63 and takes its
// count from the top of the tag:
//     bit  63      1
//     bits 62..57  frame count, 1 .. 63 (the field is 0 in every whole command: 0 reads as 64)
//     bits 56..32  tag, 1 .. 2^25 - 1
//     bits 31..0   frame offset, any value: nothing here assumes a multiple of 64 or of 4
// The choice: the offset keeps all its 32 bits and the whole command all its tag bits, so the 2 GB window (kWindowMaxOff) and
// the rebase mark of whole-buffer callers (PersistSession::rebase_at, 2^30 commands) stay where they were. The price is paid only
// by calls that carry a partial command: such a call needs every tag of the call below 2^25 (kPartialRebaseAt), or the session
// is flushed and renumbered from 0 first — one session start, microseconds. 2^25 commands are 9.3 hours of 48-frame calls at
// 48 kHz (6.2 hours at 32 frames, 11.6 hours of 120-frame packets, two commands each); whole commands beyond that tag stay legal
// in the same numbering, they are simply never followed by a partial one without the renumbering.
#pragma once

namespace namhip
{
namespace session
{
constexpr int kCmdFrames = 64; // frames of a whole command (plan.h: kBlock)
constexpr unsigned long long kPartialBit = 1ull << 63;
constexpr int kCountShift = 57; // the count field: bits 62..57
constexpr unsigned kPartialTagBits = 25;
constexpr unsigned kPartialTagMax = (1u << kPartialTagBits) - 1u; // highest tag a partial command can carry
constexpr unsigned kWholeTagMax = 0x7fffffffu; // highest tag of a whole command (bit 31: the "left" flag of the completion words)
constexpr unsigned kOffMax = 0xffffffffu; // the encoding's own limit on the frame offset
constexpr long kWindowMaxOff = 0x1fff0000l; // what the host allows: the kernels address a session's window within 2 GB
// a call with a partial command is refused by the current numbering when its commands would reach this count (api_session.cpp
// uses min(rebase_at, this) for such calls): the call's last tag is then at most kPartialTagMax
constexpr unsigned kPartialRebaseAt = 1u << kPartialTagBits;

struct Command
{
  unsigned tag; // the command's number, from 1
  unsigned off; // frame offset in the window
  int n; // frames, 1 .. 64
};

// 1 <= n <= 64; n < 64 needs tag <= kPartialTagMax. A 64-frame command is `(tag << 32) | off`, bit for bit.
constexpr unsigned long long encode(unsigned tag, unsigned off, int n)
{
  return n == kCmdFrames ? ((unsigned long long)tag << 32) | off
                         : kPartialBit | ((unsigned long long)(unsigned)n << kCountShift) | ((unsigned long long)(tag & kPartialTagMax) << 32) | off;
}
// the same from the word's upper half (what a wavefront keeps in a scalar register)
constexpr unsigned tag_of_hi(unsigned hi)
{
  return (hi & 0x80000000u) ? (hi & kPartialTagMax) : hi;
}
constexpr int frames_of_hi(unsigned hi)
{
  return (hi & 0x80000000u) ? (int)((hi >> (kCountShift - 32)) & 63u) : kCmdFrames;
}
constexpr Command decode(unsigned long long word)
{
  return Command{tag_of_hi((unsigned)(word >> 32)), (unsigned)word, frames_of_hi((unsigned)(word >> 32))};
}

// A call of n_frames is n_frames / 64 whole commands, then one partial command if frames are left over.
constexpr int command_count(int n_frames)
{
  return n_frames <= 0 ? 0 : (n_frames + kCmdFrames - 1) / kCmdFrames;
}
constexpr bool has_partial(int n_frames)
{
  return n_frames > 0 && n_frames % kCmdFrames != 0;
}
// command i of the call, 0 <= i < command_count(n_frames): where it starts in the call's buffer, how many frames it holds
constexpr int command_offset(int i)
{
  return i * kCmdFrames;
}
constexpr int command_frames(int n_frames, int i)
{
  return n_frames - i * kCmdFrames < kCmdFrames ? n_frames - i * kCmdFrames : kCmdFrames;
}
// Does the call fit the current numbering? `seq`: commands submitted so far, `rebase_at`: the session's own mark. False: the
// session is flushed and renumbered before the call (a call is never split across sessions).
constexpr unsigned rebase_mark(int n_frames, unsigned rebase_at)
{
  return has_partial(n_frames) && kPartialRebaseAt < rebase_at ? kPartialRebaseAt : rebase_at;
}
constexpr bool call_fits(unsigned seq, int n_frames, unsigned rebase_at)
{
  return seq + (unsigned)command_count(n_frames) < rebase_mark(n_frames, rebase_at);
}
} // namespace session
} // namespace namhip
