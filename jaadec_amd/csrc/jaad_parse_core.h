// The frame-local part of the AAC-LC parse (mono / stereo), written once for the host and the
// device: plain C++ under a host compiler, __host__ __device__ under hipcc.  It restates
// read_ics_info / read_ics / parse_frame_body of jaad_parse.cpp for channel configurations 1 and
// 2 without SBR -- the same reads, the same checks in the same order, hence the same status for
// the same bytes -- but keeps nothing between frames: in place of the parser's window_shape_prev
// and static PNS LCG it reports, per channel-frame, the window shape the frame left behind (when
// its shape bit was read) and how many LCG steps its noise bands took.  A link pass (lcg_jump,
// link_* below) turns those into jaad_ics_info.window_shape_prev / pns_state along a run.
// tools/gparse_diff.cpp holds this file and jaad_parse.cpp together (tests/test_gparse_core.py).
// For SBR configurations parse_frame_sbr stops where a frame's SBR payload begins and tail_dword
// cuts what is left of the frame out for the host (tools/gparse_sbr_diff.cpp,
// tests/test_gparse_sbr_core.py).
//
// No allocation, no exceptions, no statics; every loop is bounded by the bits left or a band
// count.  Tables come in as one flat image of 32-bit words (jaad_gparse_image.h builds it).
#pragma once
#include <stdint.h>

#include "../../include/jaad_gpu.h"

#if defined(__HIPCC__)
#define JAAD_PC __host__ __device__ inline
#else
#define JAAD_PC inline
#endif

namespace jaad {
namespace pcore {

// ---- table image (32-bit words) ----------------------------------------------------------------
//   [0, 48)     12 books (0..10: spectral codebooks 1..11, 11: scalefactors) x {maxlen, pbits, first
//               entry word, 0}
//   [48, 100)   swb_offset of the long window at this sample rate (count + 1 entries, rest 1024)
//   [100, 116)  swb_offset of the short window (count + 1 entries, rest 128)
//   [116, 180)  LCG power table: (a_k, c_k) with x -> a_k * x + c_k equal to 2^k LCG steps
//   [180, ...)  Lut::build's primary / secondary tables of each book.  An entry is
//               0xFFFFFFFF (no codeword), 0x80000000 | word offset of a secondary table (from the
//               book's first entry), or len << 16 | values: four 4-bit two's complement values for
//               the quad books (value j in bits 4j..4j+3), two 8-bit ones for the pair books, the
//               scalefactor delta index (0..120) for the scalefactor book.
constexpr int kImgBooks = 0, kImgSwbLong = 48, kImgSwbShort = 100, kImgLcg = 116, kImgEntries = 180;
constexpr int kBookSf = 11;
constexpr uint32_t kNoCode = 0xFFFFFFFFu;

struct Cfg {
    const uint32_t* img;
    int nswb_l, nswb_s;  // scalefactor band counts of the long / short window
    int stereo;          // 1: one CPE per frame (channel_config 2), 0: one SCE
    int tns_spec;        // cfg.tns_mode == JAAD_TNS_SPEC: the pulse tool is applied
};

// ---- bit reader --------------------------------------------------------------------------------
// MSB first over the frame's bytes, the next bits held in a 64-bit window (BitReader::Window of
// jaad_parse_internal.h): bits at or past the frame's end read as zero, left() tells where the
// reference would throw EOSException.  Src::be64(byte) returns the 8 bytes at that offset from
// the frame's start, big endian; what it returns past the frame's end does not matter (masked
// here), it only must not fault.
template <class Src>
struct Bits {
    Src src;
    int64_t end, pos;
    uint64_t buf;
    int cnt;
    JAAD_PC Bits(const Src& s, uint64_t bytes) : src(s), end((int64_t)(bytes * 8)), pos(0), buf(0), cnt(0) {}
    JAAD_PC int64_t left() const { return end - pos; }
    JAAD_PC bool overrun() const { return pos > end; }
    JAAD_PC void refill()
    {
        if (pos >= end) {
            buf = 0;
            cnt = 64;
            return;
        }
        const int sh = (int)(pos & 7);
        uint64_t w = src.be64((uint64_t)(pos >> 3)) << sh;
        cnt = 64 - sh;
        const int64_t keep = end - pos;
        if (keep < cnt) w &= ~(~0ull >> keep);
        buf = w;
    }
    JAAD_PC void need(int n)  // n <= 57
    {
        if (cnt < n) refill();
    }
    JAAD_PC uint32_t peek(int n) const { return n > 0 ? (uint32_t)(buf >> (64 - n)) : 0u; }  // after need(n), n <= 32
    JAAD_PC void skip(int64_t n)
    {
        if (n <= 0) return;
        pos += n;
        if (n >= cnt) {
            cnt = 0;
            buf = 0;
        } else {
            buf <<= n;
            cnt -= (int)n;
        }
    }
    JAAD_PC uint32_t read(int n)
    {
        need(n);
        const uint32_t v = peek(n);
        skip(n);
        return v;
    }
    JAAD_PC void byte_align() { skip(((pos + 7) & ~(int64_t)7) - pos); }
};

// Lut::decode: 0 and the entry, or -1 (no codeword) / -2 (the bitstream ended)
template <class B>
JAAD_PC int huff(B& br, const uint32_t* e, int maxlen, int pbits, int extra, uint32_t& out)
{
    br.need(maxlen + extra);
    const uint32_t peek = br.peek(maxlen);
    uint32_t ent = e[peek >> (maxlen - pbits)];
    if (ent != kNoCode && (ent & 0x80000000u)) ent = e[(ent & 0x7FFFFFFFu) + (peek & ((1u << (maxlen - pbits)) - 1u))];
    if (ent == kNoCode) return br.left() < maxlen ? -2 : -1;
    const int len = (int)(ent >> 16);
    if (br.left() < len) return -2;
    br.skip(len);
    out = ent;
    return 0;
}

// ---- what one channel-frame reports ------------------------------------------------------------
struct ChInfo {
    uint8_t seq, shape, max_sfb, grouping, flags;
    uint8_t shape_valid;   // the window_shape bit was read: the channel's shape is `shape` from here on
    uint32_t noise_steps;  // LCG steps taken: all noise bins of a parsed channel, those
                           // decodeSpectralData had passed when the bitstream ended (JAAD_ERR_EOS)
};
struct FrameInfo {
    ChInfo ch[2];
    uint64_t ms[2];
};

struct IcsI {
    int seq, shape, max_sfb, grouping, ngroups;
    uint32_t glen;  // group g's length in bits 4g..4g+3
};

typedef uint32_t __attribute__((may_alias)) u32_alias;
typedef uint64_t __attribute__((may_alias)) u64_alias;

// read_ics_info of jaad_parse.cpp
template <class B>
JAAD_PC int read_ics_info(B& br, const Cfg& C, IcsI& I, ChInfo* shape_state)
{
    if (br.left() < 4) return JAAD_ERR_EOS;
    br.skip(1);
    I.seq = (int)br.read(2);
    I.shape = (int)br.read(1);
    if (shape_state) {
        shape_state->shape_valid = 1;
        shape_state->shape = (uint8_t)I.shape;
    }
    I.ngroups = 1;
    I.glen = 1;
    I.grouping = 0;
    if (I.seq == JAAD_EIGHT_SHORT_SEQUENCE) {
        if (br.left() < 11) return JAAD_ERR_EOS;
        I.max_sfb = (int)br.read(4);
        const uint32_t bits = br.read(7);
        for (int i = 0; i < 7; i++) {
            if ((bits >> (6 - i)) & 1u) {
                I.glen += 1u << (4 * (I.ngroups - 1));
                I.grouping |= 1 << i;
            } else {
                I.glen |= 1u << (4 * I.ngroups);
                I.ngroups++;
            }
        }
        if (I.max_sfb > C.nswb_s) return JAAD_ERR_BITSTREAM;
    } else {
        if (br.left() < 6) return JAAD_ERR_EOS;
        I.max_sfb = (int)br.read(6);
        if (br.left() < 1) return JAAD_ERR_EOS;
        if (br.read(1)) return JAAD_ERR_UNSUPPORTED;
        if (I.max_sfb > C.nswb_l) return JAAD_ERR_BITSTREAM;
    }
    return br.overrun() ? JAAD_ERR_EOS : JAAD_OK;
}

// read_ics of jaad_parse.cpp.  cb / sf are zeroed 128-byte rows, q a zeroed, 8-byte aligned
// 1024-value row, T a zeroed jaad_tns or NULL (parsed and dropped).
template <class B>
JAAD_PC int read_ics(B& br, const Cfg& C, bool common_window, IcsI& I, ChInfo& R, uint8_t* cb, uint8_t* sf, int16_t* q,
                     jaad_tns* T)
{
    const uint32_t* img = C.img;
    if (br.left() < 8) return JAAD_ERR_EOS;
    const int global_gain = (int)br.read(8);
    if (!common_window) {
        const int st = read_ics_info(br, C, I, &R);
        if (st) return st;
    }
    const bool is_short = I.seq == JAAD_EIGHT_SHORT_SEQUENCE;
    const uint32_t* swb = img + (is_short ? kImgSwbShort : kImgSwbLong);
    const int nswb = is_short ? C.nswb_s : C.nswb_l;
    const int max_sfb = I.max_sfb;

    // ---- section data
    {
        const int bits = is_short ? 3 : 5, esc = (1 << bits) - 1;
        int idx = 0;
        for (int g = 0; g < I.ngroups; g++) {
            for (int k = 0; k < max_sfb;) {
                int end = k;
                if (br.left() < 4) return JAAD_ERR_EOS;
                const int c = (int)br.read(4);
                if (c == 12) return JAAD_ERR_BITSTREAM;
                int incr;
                do {
                    if (br.left() < bits) return JAAD_ERR_EOS;
                    incr = (int)br.read(bits);
                    end += incr;
                } while (incr == esc);
                if (end > max_sfb) return JAAD_ERR_BITSTREAM;
                for (; k < end; k++, idx++) cb[idx] = (uint8_t)c;
            }
        }
    }
    // ---- scalefactors (a section's bands share its codebook: band by band is the same walk)
    int has_pns = 0, has_is = 0;
    {
        const int maxlen = (int)img[kBookSf * 4], pbits = (int)img[kBookSf * 4 + 1];
        const uint32_t* e = img + img[kBookSf * 4 + 2];
        int off0 = global_gain, off1 = global_gain - 90, off2 = 0;
        bool noise_flag = true;
        const int nb = I.ngroups * max_sfb;
        for (int idx = 0; idx < nb; idx++) {
            const int c = cb[idx];
            if (c == JAAD_ZERO_HCB) continue;
            int d;
            if (c == JAAD_NOISE_HCB && noise_flag) {
                if (br.left() < 9) return JAAD_ERR_EOS;
                d = (int)br.read(9) - 256;
                noise_flag = false;
            } else {
                uint32_t ent;
                const int r = huff(br, e, maxlen, pbits, 0, ent);
                if (r < 0) return r == -2 ? JAAD_ERR_EOS : JAAD_ERR_BITSTREAM;
                d = (int)(ent & 0xFFu) - 60;
            }
            if (c == JAAD_INTENSITY_HCB || c == JAAD_INTENSITY_HCB2) {
                off2 += d;
                const int t = off2 < -155 ? -155 : (off2 > 100 ? 100 : off2);
                sf[idx] = (uint8_t)(100 - t);
                has_is = 1;
            } else if (c == JAAD_NOISE_HCB) {
                off1 += d;
                const int t = off1 < -100 ? -100 : (off1 > 155 ? 155 : off1);
                sf[idx] = (uint8_t)(t + 100);
                has_pns = 1;
            } else {
                off0 += d;
                if (off0 > 255) return JAAD_ERR_BITSTREAM;
                if (off0 < 0) return JAAD_ERR_BITSTREAM;
                sf[idx] = (uint8_t)off0;
            }
        }
    }
    // ---- pulse data: offset in bits 0..11, amplitude in bits 12..15 of each 16-bit field
    int pulse_n = 0;
    uint64_t pulses = 0;
    if (br.left() < 1) return JAAD_ERR_EOS;
    if (br.read(1)) {
        if (is_short) return JAAD_ERR_BITSTREAM;
        if (br.left() < 8) return JAAD_ERR_EOS;
        const int count = (int)br.read(2) + 1;
        const int start = (int)br.read(6);
        if (start >= nswb) return JAAD_ERR_BITSTREAM;
        int offs = (int)swb[start];
        for (int i = 0; i < count; i++) {
            if (br.left() < 9) return JAAD_ERR_EOS;
            offs += (int)br.read(5);
            const int amp = (int)br.read(4);
            pulses |= (uint64_t)((uint32_t)offs | ((uint32_t)amp << 12)) << (16 * i);
            if (i > 0 && offs > 1023) return JAAD_ERR_BITSTREAM;
        }
        pulse_n = count;
    }
    // ---- TNS data
    if (br.left() < 1) return JAAD_ERR_EOS;
    const bool tns_present = br.read(1) != 0;
    if (tns_present) {
        const int nwin = is_short ? 8 : 1;
        const int b0 = is_short ? 1 : 2, b1 = is_short ? 4 : 6, b2 = is_short ? 3 : 5;
        int n_filters = 0;
        for (int w = 0; w < nwin; w++) {
            if (br.left() < b0) return JAAD_ERR_EOS;
            const int nf = (int)br.read(b0);
            if (!nf) continue;
            if (br.left() < 1) return JAAD_ERR_EOS;
            const int res = (int)br.read(1);
            for (int f = 0; f < nf; f++) {
                if (br.left() < b1 + b2) return JAAD_ERR_EOS;
                if (n_filters >= 8) return JAAD_ERR_BITSTREAM;
                jaad_tns_filter* F = T ? &T->filt[n_filters] : nullptr;
                n_filters++;
                if (T) T->n_filters = (uint8_t)n_filters;
                const int length = (int)br.read(b1);
                const int order = (int)br.read(b2);
                if (F) {
                    F->window = (uint8_t)w;
                    F->length = (uint8_t)length;
                }
                if (order > 20) return JAAD_ERR_BITSTREAM;
                int flags = res << 1;
                if (F) F->order = (uint8_t)order;
                if (order) {
                    if (br.left() < 2) return JAAD_ERR_EOS;
                    const int dir = (int)br.read(1), comp = (int)br.read(1);
                    const int len = res + 3 - comp;
                    flags = dir | (res << 1) | (comp << 2);
                    for (int i = 0; i < order; i++) {
                        if (br.left() < len) return JAAD_ERR_EOS;
                        const uint32_t v = br.read(len);
                        if (F) F->coef[i] = (uint8_t)v;
                    }
                }
                if (F) F->flags = (uint8_t)flags;
            }
        }
    }
    // ---- gain control: AAC SSR only
    if (br.left() < 1) return JAAD_ERR_EOS;
    if (br.read(1)) return JAAD_ERR_UNSUPPORTED;

    // ---- spectral data.  swb offsets are multiples of 4, so a quad is one aligned 8-byte store
    // and a pair one aligned 4-byte store into the zeroed row.
    // The walk is decodeSpectralData's -- groups, bands, the group's windows, the band's codewords,
    // in that order -- written as one loop over codewords with the position kept in variables: on
    // the device the lanes of a wave (one frame each) then meet once per codeword, not at the end
    // of every band, where each would wait for the longest band among them.
    uint32_t noise_steps = 0;
    {
        int g = 0, s = 0, idx = 0, group_off = 0, w = 0, k = 0;
        int gl = (int)(I.glen & 15u);
        int c = 0, lo = 0, width = 0, maxlen = 0, pbits = 0;
        const uint32_t* e = img;
        bool pair = false, unsigned_cb = false, in_band = false;
        for (;;) {
            while (!in_band && g < I.ngroups) {  // the next band with coded values
                if (s >= max_sfb) {
                    group_off += gl << 7;
                    g++;
                    s = 0;
                    gl = (int)((I.glen >> (4 * (g & 7))) & 15u);
                    continue;
                }
                c = cb[idx];
                lo = (int)swb[s];
                width = (int)swb[s + 1] - lo;
                if (c == JAAD_ZERO_HCB || c == JAAD_INTENSITY_HCB || c == JAAD_INTENSITY_HCB2) {
                    s++, idx++;
                    continue;
                }
                if (c == JAAD_NOISE_HCB) {
                    noise_steps += (uint32_t)(gl * width);
                    s++, idx++;
                    continue;
                }
                if (c > JAAD_ESCAPE_HCB) return JAAD_ERR_BITSTREAM;
                maxlen = (int)img[(c - 1) * 4];
                pbits = (int)img[(c - 1) * 4 + 1];
                e = img + img[(c - 1) * 4 + 2];
                pair = c >= JAAD_FIRST_PAIR_HCB;
                unsigned_cb = c == 3 || c == 4 || c >= 7;
                w = k = 0;
                in_band = true;
            }
            if (!in_band) break;
            const int off = group_off + w * 128 + lo;
            uint32_t ent;
            const int r = huff(br, e, maxlen, pbits, 4, ent);
            if (r < 0) {
                if (r != -2) return JAAD_ERR_BITSTREAM;
                R.noise_steps = noise_steps;
                return JAAD_ERR_EOS;
            }
            int v[4];
            if (pair) {
                v[0] = (int)(int8_t)(ent & 0xFFu);
                v[1] = (int)(int8_t)((ent >> 8) & 0xFFu);
                v[2] = v[3] = 0;
            } else {
                for (int j = 0; j < 4; j++) v[j] = (int)(((ent >> (4 * j)) & 15u) ^ 8u) - 8;
            }
            if (unsigned_cb) {  // one sign bit per nonzero value
                int nz = 0;
                for (int j = 0; j < 4; j++) nz += v[j] != 0;
                if (br.left() < nz) {
                    R.noise_steps = noise_steps;
                    return JAAD_ERR_EOS;
                }
                uint32_t bits = nz ? br.read(nz) << (32 - nz) : 0u;
                for (int j = 0; j < 4; j++) {
                    const uint32_t has = v[j] != 0;
                    const bool neg = (bits >> 31) & has;
                    bits <<= has;
                    v[j] = neg ? -v[j] : v[j];
                }
            }
            if (c == JAAD_ESCAPE_HCB)
                for (int j = 0; j < 2; j++) {
                    if (v[j] != 16 && v[j] != -16) continue;
                    br.need(9 + 13);
                    const int avail = br.left() < 9 ? (int)br.left() : 9;
                    const int ones = avail > 0 ? __builtin_clz(~(br.peek(avail) << (32 - avail))) : 0;
                    if (ones >= 9) return JAAD_ERR_BITSTREAM;
                    if (ones == avail) {
                        R.noise_steps = noise_steps;
                        return JAAD_ERR_EOS;
                    }
                    br.skip(ones + 1);
                    const int n = 4 + ones;
                    if (br.left() < n) {
                        R.noise_steps = noise_steps;
                        return JAAD_ERR_EOS;
                    }
                    const int m = (int)br.read(n) | (1 << n);
                    if (m > 8190) return JAAD_ERR_BITSTREAM;
                    v[j] = v[j] < 0 ? -m : m;
                }
            const uint32_t w0 = ((uint32_t)v[0] & 0xFFFFu) | ((uint32_t)v[1] << 16);
            if (pair) {
                *reinterpret_cast<u32_alias*>(q + off + k) = w0;
            } else {
                const uint32_t w1 = ((uint32_t)v[2] & 0xFFFFu) | ((uint32_t)v[3] << 16);
                *reinterpret_cast<u64_alias*>(q + off + k) = (uint64_t)w0 | ((uint64_t)w1 << 32);
            }
            k += pair ? 2 : 4;
            if (k >= width) {
                k = 0;
                if (++w >= gl) {
                    in_band = false;
                    s++, idx++;
                }
            }
        }
    }
    if (br.overrun()) return JAAD_ERR_EOS;
    if (C.tns_spec)
        for (int i = 0; i < pulse_n; i++) {
            const int k = (int)((pulses >> (16 * i)) & 0xFFFu), amp = (int)((pulses >> (16 * i + 12)) & 15u);
            if (k > 1023) return JAAD_ERR_BITSTREAM;
            const int v = q[k] > 0 ? q[k] + amp : q[k] - amp;
            if (v > 8190 || v < -8190) return JAAD_ERR_BITSTREAM;
            q[k] = (int16_t)v;
        }
    R.seq = (uint8_t)I.seq;
    R.shape = (uint8_t)I.shape;
    R.max_sfb = (uint8_t)max_sfb;
    R.grouping = (uint8_t)I.grouping;
    R.flags = (uint8_t)((has_pns ? JAAD_ICS_HAS_PNS : 0) | (has_is ? JAAD_ICS_HAS_IS : 0) | (tns_present ? JAAD_ICS_TNS : 0) |
                        (common_window ? JAAD_ICS_COMMON_WINDOW : 0));
    R.noise_steps = noise_steps;
    return JAAD_OK;
}

template <class B>
JAAD_PC int skip_dse(B& br)
{
    if (br.left() < 9) return JAAD_ERR_EOS;
    const bool align = br.read(1) != 0;
    int count = (int)br.read(8);
    if (count == 255) {
        if (br.left() < 8) return JAAD_ERR_EOS;
        count += (int)br.read(8);
    }
    if (align) br.byte_align();
    if (br.left() < 8 * count) return JAAD_ERR_EOS;
    br.skip(8 * count);
    return JAAD_OK;
}

template <class B>
JAAD_PC int skip_pce(B& br)
{
    if (br.left() < 2 + 4 + 4 + 4 + 4 + 2 + 3 + 4) return JAAD_ERR_EOS;
    br.skip(2 + 4);
    const int nfront = (int)br.read(4), nside = (int)br.read(4), nback = (int)br.read(4);
    const int nlfe = (int)br.read(2), nassoc = (int)br.read(3), ncc = (int)br.read(4);
    if (br.read(1)) br.skip(4);
    if (br.read(1)) br.skip(4);
    if (br.read(1)) br.skip(3);
    br.skip(5 * (nfront + nside + nback) + 4 * nlfe + 4 * nassoc + 5 * ncc);
    br.byte_align();
    if (br.left() < 8) return JAAD_ERR_EOS;
    const int ncomment = (int)br.read(8);
    br.skip(8 * ncomment);
    return br.overrun() ? JAAD_ERR_EOS : JAAD_OK;
}

JAAD_PC uint32_t bitrev32(uint32_t v)
{
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
}

// parse_frame_body of jaad_parse.cpp for one SCE or one CPE per frame, no SBR, no CCE output:
// the element loop with the frame's status.  `out` hands out the rows each channel is parsed
// into (the contract of read_ics) and is told when a channel's rows are complete:
//   uint8_t* cb(int ch); uint8_t* sf(int ch); int16_t* q(int ch); jaad_tns* tns(int ch);
//   void done(int ch);
// F is valid for status 0 and, as far as shape_valid / noise_steps go, for JAAD_ERR_EOS.
// kSbr (an SBR configuration, parse_frame_sbr below): the first FIL element after the channel
// element that holds an SBR payload (count != 0, its bytes are there, extension type 13 or 14) ends
// the walk with JAAD_OK and tail_bit = the bit position of that FIL's id_syn_ele; what follows from
// there on -- the frame's tail -- is the host's to parse.  tail_bit stays -1 otherwise.
template <bool kSbr, class B, class Out>
JAAD_PC int parse_frame_t(B& br, const Cfg& C, Out& out, FrameInfo& F, int64_t& tail_bit)
{
    tail_bit = -1;
    for (int c = 0; c < 2; c++) {
        F.ch[c].seq = F.ch[c].shape = F.ch[c].max_sfb = F.ch[c].grouping = F.ch[c].flags = F.ch[c].shape_valid = 0;
        F.ch[c].noise_steps = 0;
    }
    F.ms[0] = F.ms[1] = 0;
    bool have_channels = false;
    int elem = 0;
    for (;;) {
        if (br.left() < 3) return JAAD_ERR_EOS;
        const int64_t at = br.pos;
        const int id = (int)br.read(3);
        if (id == 7) break;
        if (id == 6) {  // FIL
            if (br.left() < 4) return JAAD_ERR_EOS;
            int count = (int)br.read(4);
            if (count == 15) {
                if (br.left() < 8) return JAAD_ERR_EOS;
                count += (int)br.read(8) - 1;
            }
            if (!count) continue;
            if (br.left() < 8 * count) return JAAD_ERR_EOS;
            br.need(4);
            const int type = (int)br.peek(4);
            br.skip(8 * count);
            if ((type == 13 || type == 14) && have_channels) {
                if (!kSbr) return JAAD_ERR_UNSUPPORTED;  // SBR payload, core config
                tail_bit = at;
                return JAAD_OK;
            }
            continue;
        }
        if (br.left() < 4) return JAAD_ERR_EOS;
        br.skip(4);  // element_instance_tag
        if (id == 4) {
            const int st = skip_dse(br);
            if (st) return st;
            continue;
        }
        if (id == 5) {
            const int st = skip_pce(br);
            if (st) return st;
            continue;
        }
        if (id == 2) return JAAD_ERR_UNSUPPORTED;  // CCE: no coupling output here
        if (elem >= 1 || (id == 1) != (C.stereo != 0) || id == 3) return JAAD_ERR_UNSUPPORTED;
        have_channels = true;
        if (id == 0) {
            IcsI I;
            I.seq = I.shape = I.max_sfb = I.grouping = 0;
            I.ngroups = 1;
            I.glen = 1;
            const int st = read_ics(br, C, false, I, F.ch[0], out.cb(0), out.sf(0), out.q(0), out.tns(0));
            if (st) return st;
            out.done(0);
        } else {
            if (br.left() < 1) return JAAD_ERR_EOS;
            const bool common = br.read(1) != 0;
            IcsI IL, IR;
            IL.seq = IL.shape = IL.max_sfb = IL.grouping = 0;
            IL.ngroups = 1;
            IL.glen = 1;
            IR = IL;
            bool ms_present = false;
            if (common) {
                int st = read_ics_info(br, C, IL, &F.ch[0]);
                if (st) return st;
                IR = IL;
                F.ch[1].shape_valid = 1;
                F.ch[1].shape = (uint8_t)IR.shape;
                if (br.left() < 2) return JAAD_ERR_EOS;
                const int mask = (int)br.read(2);
                const int nb = IL.ngroups * IL.max_sfb;
                if (mask == 1) {
                    if (br.left() < nb) return JAAD_ERR_EOS;
                    for (int i = 0; i < nb; i += 32) {
                        const int n = nb - i < 32 ? nb - i : 32;
                        const uint32_t v = bitrev32(br.read(n)) >> (32 - n);
                        F.ms[i >> 6] |= (uint64_t)v << (i & 63);
                    }
                } else if (mask == 2) {
                    F.ms[0] = nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
                    F.ms[1] = nb > 64 ? (nb >= 128 ? ~0ull : (1ull << (nb - 64)) - 1ull) : 0ull;
                } else if (mask == 3) {
                    return JAAD_ERR_BITSTREAM;
                }
                ms_present = mask != 0;
            }
            int st = read_ics(br, C, common, IL, F.ch[0], out.cb(0), out.sf(0), out.q(0), out.tns(0));
            if (st) return st;
            out.done(0);
            st = read_ics(br, C, common, IR, F.ch[1], out.cb(1), out.sf(1), out.q(1), out.tns(1));
            if (st) return st;
            out.done(1);
            if (ms_present) F.ch[0].flags |= JAAD_ICS_MS_PRESENT;
        }
        elem++;
    }
    if (!have_channels) return JAAD_ERR_BITSTREAM;
    return JAAD_OK;
}

template <class B, class Out>
JAAD_PC int parse_frame(B& br, const Cfg& C, Out& out, FrameInfo& F)
{
    int64_t tail_bit;
    return parse_frame_t<false>(br, C, out, F, tail_bit);
}
template <class B, class Out>
JAAD_PC int parse_frame_sbr(B& br, const Cfg& C, Out& out, FrameInfo& F, int64_t& tail_bit)
{
    return parse_frame_t<true>(br, C, out, F, tail_bit);
}

// ---- tail copy ---------------------------------------------------------------------------------
// The bits [src_bit, src_bit + nbits) of a buffer, shifted to bit 0: dword k of the copy (the bits
// 32k .. 32k + 31 of the tail, MSB first, as a big-endian value), zero from bit nbits on.
// Src::dword_be(byte) returns the big-endian dword at an aligned byte offset and reads as zero,
// without touching memory, past the buffer.
template <class Src>
JAAD_PC uint32_t tail_dword(const Src& src, uint64_t src_bit, uint64_t nbits, uint64_t k)
{
    if (32u * k >= nbits) return 0u;
    const uint64_t p = src_bit + 32u * k;
    const uint32_t at = (uint32_t)(p >> 5) * 4u, sh = (uint32_t)(p & 31u);
    uint32_t w = src.dword_be(at) << sh;
    const uint64_t rest = nbits - 32u * k;
    if (sh && rest > 32u - sh) w |= src.dword_be(at + 4u) >> (32u - sh);
    if (rest < 32u) w &= ~(0xFFFFFFFFu >> rest);
    return w;
}
// bytes of a tail in the pool: whole bytes, rounded up to 8
JAAD_PC uint32_t tail_pool_bytes(uint32_t bytes) { return (bytes + 7u) & ~7u; }

// ---- link pass ---------------------------------------------------------------------------------
// The LCG x -> 1664525 x + 1013904223 (mod 2^32) is affine, so n steps are one map (a, c).
struct Affine {
    uint32_t a, c;
};
JAAD_PC Affine affine_id()
{
    Affine m = {1u, 0u};
    return m;
}
// first f, then g
JAAD_PC Affine affine_then(Affine f, Affine g)
{
    Affine m = {g.a * f.a, g.a * f.c + g.c};
    return m;
}
JAAD_PC uint32_t affine_apply(Affine m, uint32_t x) { return m.a * x + m.c; }
// t[2k], t[2k+1] = (a, c) of 2^k steps
JAAD_PC void lcg_pow_table(uint32_t* t)
{
    uint32_t a = 1664525u, c = 1013904223u;
    for (int k = 0; k < 32; k++) {
        t[2 * k] = a;
        t[2 * k + 1] = c;
        c = c * (a + 1u);
        a = a * a;
    }
}
// n steps by binary powering over the table
JAAD_PC Affine lcg_jump(const uint32_t* t, uint32_t n)
{
    Affine m = affine_id();
    for (int k = 0; n; k++, n >>= 1)
        if (n & 1u) {
            Affine p = {t[2 * k], t[2 * k + 1]};
            m = affine_then(m, p);
        }
    return m;
}

// what the frame kernel leaves per channel-frame for the link pass
JAAD_PC uint32_t link_pack(const ChInfo& c) { return c.noise_steps | ((uint32_t)c.shape_valid << 31) | ((uint32_t)(c.shape & 1u) << 30); }
JAAD_PC uint32_t link_steps(uint32_t p) { return p & 0x3FFFFFFFu; }
JAAD_PC uint32_t link_shape(uint32_t p) { return p >> 30; }  // bit 1: valid, bit 0: shape

}  // namespace pcore
}  // namespace jaad
