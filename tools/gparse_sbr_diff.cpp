// Differential check of the split HE-AAC parse (include/jaad_gparse.h, jaad_gparse_batch_sbr) against
// the host parser (jaad_parse_frame), built for the host with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_gparse_sbr_core.py.  One side runs what the device runs,
// in scalar form: the SBR variant of the shared core (jaad_parse_core.h parse_frame_sbr) per frame,
// the link pass, an exclusive scan of the tails' pool sizes, the shared bit-shift copy (tail_dword)
// into a pool, then the host tail stage (jaad_parse_tail.h parse_tails).  The other side is a
// jaad_parser over the same frames.  Batches are windows of seed runs (valid mono SBR + PS and
// stereo SBR raw_data_blocks from the test writer), as they are and with one frame bit-flipped /
// truncated.  Required: the same status for every frame; for status 0 the same q / sf / cb / ics /
// ms_used / tns bytes; for 0 and EOS the same jaad_sbr_frame bytes; the same parser state afterwards
// (all-or-nothing as jaad_gparse_batch_sbr: seen through the records of seed frames parsed next on
// copies of both parsers).  No mutant is left out.  Also tail_dword against a bit-by-bit copy.
// Usage: gparse_sbr_diff <seeds.bin> <mutants>; seeds.bin: records of {u8 sf_index, u8 channel_config,
// u8 tns_mode, u8 ps, u8 ext_sf_index, u8 run, u32 bytes, bytes}, a run's frames in order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jaad_gparse_image.h"
#include "jaad_parse_tail.h"

using namespace jaad::pcore;

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return (uint32_t)(rs >> 11);
}

// the frame's bytes for the core's bit reader / the data buffer for tail_dword, as the device's
// DevSrc reads: aligned dwords, the buffer's last partial dword byte by byte, zero past it
struct HostSrc {
    const uint8_t* d;
    size_t n;
    uint64_t be64(uint64_t byte) const
    {
        uint64_t w = 0;
        for (size_t i = 0; i < 8; i++) w = (w << 8) | (byte + i < n ? d[byte + i] : 0u);
        return w;
    }
    uint32_t dword_be(uint32_t off) const
    {
        if (off & 3u) abort();
        uint32_t w = 0;
        for (uint32_t i = 0; i < 4; i++) w = (w << 8) | (off + i < n ? d[off + i] : 0u);
        return w;
    }
};

struct Rows {
    int16_t q[2][1024];
    uint8_t sf[2][128], cb[2][128];
    jaad_ics_info ics[2];
    jaad_tns tns[2];
    uint64_t ms[2];
    void clear() { memset(this, 0, sizeof *this); }
};
struct RowsOut {
    Rows* r;
    uint8_t* cb(int c) { return r->cb[c]; }
    uint8_t* sf(int c) { return r->sf[c]; }
    int16_t* q(int c) { return r->q[c]; }
    jaad_tns* tns(int c) { return &r->tns[c]; }
    void done(int) {}
};

struct Stream {  // one run: the host parser, and the parser the split side carries
    jaad_stream_cfg cfg;
    int run = 0;
    jaad_parser *H = nullptr, *S = nullptr;
    std::vector<uint32_t> img;
    Cfg C;
    std::vector<std::vector<std::vector<uint8_t>>> runs;
};

static int fails = 0;
static void fail(const char* what, int it)
{
    if (fails++ < 20) fprintf(stderr, "MISMATCH %s (iteration %d)\n", what, it);
}

static int host_frame(jaad_parser* P, const std::vector<uint8_t>& d, Rows& h, jaad_sbr_frame& sbr)
{
    h.clear();
    jaad_frame_out o;
    memset(&o, 0, sizeof o);
    o.q = h.q[0];
    o.sf = h.sf[0];
    o.cb = h.cb[0];
    o.ics = h.ics;
    o.ms_used = h.ms;
    o.tns = h.tns;
    o.sbr = &sbr;
    // an exact-size heap copy: a read past the frame is an AddressSanitizer report
    uint8_t* data = d.empty() ? nullptr : (uint8_t*)malloc(d.size());
    if (data) memcpy(data, d.data(), d.size());
    const int st = jaad_parse_frame(P, data, d.size(), &o);
    free(data);
    return st;
}

static int counts[16], tail_counts[16];

// One batch (one run) through both sides.  count: the frame whose final status is counted (-1: none).
// Returns 0 when every frame ended 0 or EOS.
static int both(Stream& T, const std::vector<std::vector<uint8_t>>& frames, int count, int it)
{
    const int nch = T.C.stereo ? 2 : 1;
    const uint32_t nf = (uint32_t)frames.size();
    // ---- host: frame by frame on a copy, committed when the batch succeeds
    std::vector<Rows> h(nf);
    std::vector<jaad_sbr_frame> hs(nf);
    std::vector<int8_t> hst(nf);
    jaad_parser* Hw = nullptr;
    if (jaad_parser_clone(T.H, &Hw)) abort();
    int want = 0;
    for (uint32_t f = 0; f < nf; f++) {
        memset(&hs[f], 0, sizeof hs[f]);
        hst[f] = (int8_t)host_frame(Hw, frames[f], h[f], hs[f]);
        if (!want && hst[f] != JAAD_OK && hst[f] != JAAD_ERR_EOS) want = hst[f];
    }
    if (!want) jaad_parser_copy(T.H, Hw);
    jaad_parser_destroy(Hw);
    // ---- the device's part, scalar: all frames lie in one buffer, as in a batch
    std::vector<uint8_t> blob;
    std::vector<uint32_t> off(nf);
    for (uint32_t f = 0; f < nf; f++) {
        off[f] = (uint32_t)blob.size();
        blob.insert(blob.end(), frames[f].begin(), frames[f].end());
    }
    uint8_t* data = (uint8_t*)malloc(blob.size() ? blob.size() : 1);
    if (!blob.empty()) memcpy(data, blob.data(), blob.size());
    std::vector<Rows> c(nf);
    std::vector<int8_t> cst(nf);
    std::vector<uint32_t> info(2 * nf, 0u), tsrc(nf, 0u), pool_off(nf + 1, 0u);
    jaad_gparse_state cs;
    memset(&cs, 0, sizeof cs);
    jaad::parse::parser_core_state(T.S, cs.pns_state, cs.window_shape);
    for (uint32_t f = 0; f < nf; f++) {
        c[f].clear();
        RowsOut out{&c[f]};
        FrameInfo F;
        HostSrc src{data + off[f], frames[f].size()};
        Bits<HostSrc> br(src, frames[f].size());
        int64_t tail_bit;
        const int sc = parse_frame_sbr(br, T.C, out, F, tail_bit);
        cst[f] = (int8_t)sc;
        if (sc == JAAD_OK && tail_bit >= 0) {
            tsrc[f] = off[f] + (uint32_t)(tail_bit >> 3);
            info[2 * f] = (uint32_t)frames[f].size() - (uint32_t)(tail_bit >> 3);
            info[2 * f + 1] = (uint32_t)(tail_bit & 7);
        }
        if (sc != JAAD_OK && sc != JAAD_ERR_EOS) continue;
        for (int ch = 0; ch < nch; ch++) {  // the link pass
            const ChInfo& I = F.ch[ch];
            if (sc == JAAD_OK) {
                jaad_ics_info& ic = c[f].ics[ch];
                ic.window_sequence = I.seq;
                ic.window_shape = I.shape;
                ic.window_shape_prev = cs.window_shape[ch];
                ic.max_sfb = I.max_sfb;
                ic.grouping = I.grouping;
                ic.flags = I.flags;
                ic.pns_state = cs.pns_state;
            }
            cs.pns_state = affine_apply(lcg_jump(&T.img[kImgLcg], I.noise_steps), cs.pns_state);
        }
        for (int ch = 0; ch < nch; ch++)
            if (F.ch[ch].shape_valid) cs.window_shape[ch] = F.ch[ch].shape;
        c[f].ms[0] = F.ms[0];
        c[f].ms[1] = F.ms[1];
    }
    for (uint32_t f = 0; f < nf; f++) pool_off[f + 1] = pool_off[f] + tail_pool_bytes(info[2 * f]);
    const size_t pool_bytes = (size_t)pool_off[nf] + 8;
    uint8_t* pool = (uint8_t*)malloc(pool_bytes);  // every byte written below, as the gather kernel does
    HostSrc whole{data, blob.size()};
    for (uint32_t f = 0; f < nf; f++)
        for (uint32_t k = 0; k < tail_pool_bytes(info[2 * f]) / 4; k++) {
            const uint32_t w = tail_dword(whole, (uint64_t)tsrc[f] * 8 + info[2 * f + 1], (uint64_t)info[2 * f] * 8 - info[2 * f + 1], k);
            const uint8_t b[4] = {(uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w};
            memcpy(pool + pool_off[f] + 4 * k, b, 4);
        }
    memset(pool + pool_off[nf], 0, 8);
    // ---- the host tail stage
    const uint32_t fb[2] = {0, nf};
    jaad::parse::TailBatch tb;
    tb.n_frames = nf;
    tb.n_runs = 1;
    tb.frame_begin = fb;
    tb.core_status = cst.data();
    tb.pool_off = pool_off.data();
    tb.tail_info = info.data();
    tb.pool = pool;
    tb.core_state = &cs;
    std::vector<jaad_sbr_frame> ss(nf);
    std::vector<int8_t> sst(nf);
    const int got = jaad::parse::parse_tails(&T.S, tb, ss.data(), sst.data(), 2);
    free(pool);
    free(data);
    // ---- compare
    if (got != want) {
        fprintf(stderr, "batch status: split %d host %d\n", got, want);
        fail("batch status", it);
    }
    // A frame the tail stage refuses has moved the device's link pass (its core parsed) but not the
    // host parser: from there on the batch's pns_state / window_shape_prev differ.  That batch has
    // failed (jaad_gparse.h: its records are unspecified); everything else is still compared.
    bool link_off = false;
    for (uint32_t f = 0; f < nf; f++) {
        if (link_off && sst[f] == JAAD_OK && hst[f] == JAAD_OK)
            for (int ch = 0; ch < nch; ch++) {
                c[f].ics[ch].pns_state = h[f].ics[ch].pns_state;
                c[f].ics[ch].window_shape_prev = h[f].ics[ch].window_shape_prev;
            }
        if (cst[f] == JAAD_OK && sst[f] != JAAD_OK && sst[f] != JAAD_ERR_EOS) link_off = true;
        if (sst[f] != hst[f]) {
            fprintf(stderr, "frame %u status: split %d (core %d) host %d\n", f, sst[f], cst[f], hst[f]);
            fail("status", it);
            continue;
        }
        if ((int)f == count) {
            counts[-sst[f] < 16 ? -sst[f] : 15]++;
            if (cst[f] == JAAD_OK && info[2 * f]) tail_counts[-sst[f] < 16 ? -sst[f] : 15]++;
        }
        if (sst[f] == JAAD_OK) {
            if (memcmp(h[f].q, c[f].q, sizeof(int16_t) * 1024 * nch)) fail("q", it);
            if (memcmp(h[f].sf, c[f].sf, sizeof h[f].sf)) fail("sf", it);
            if (memcmp(h[f].cb, c[f].cb, sizeof h[f].cb)) fail("cb", it);
            if (memcmp(h[f].ics, c[f].ics, sizeof(jaad_ics_info) * nch)) fail("ics", it);
            if (nch == 2 && memcmp(h[f].ms, c[f].ms, sizeof h[f].ms)) fail("ms_used", it);
            if (memcmp(h[f].tns, c[f].tns, sizeof(jaad_tns) * nch)) fail("tns", it);
        }
        if ((sst[f] == JAAD_OK || sst[f] == JAAD_ERR_EOS) && memcmp(&hs[f], &ss[f], sizeof hs[f])) fail("sbr record", it);
    }
    return want;
}

// the state both parsers are in, seen through the records of seed frames parsed next on copies
static void same_state(Stream& T, const std::vector<std::vector<uint8_t>>& probe, int it)
{
    jaad_parser *a = nullptr, *b = nullptr;
    if (jaad_parser_clone(T.H, &a) || jaad_parser_clone(T.S, &b)) abort();
    if (jaad_parser_pns_state(a) != jaad_parser_pns_state(b)) fail("pns state after the batch", it);
    static Rows ra, rb;
    for (size_t f = 0; f < probe.size(); f++) {
        jaad_sbr_frame sa, sb;
        memset(&sa, 0, sizeof sa);
        memset(&sb, 0, sizeof sb);
        const int x = host_frame(a, probe[f], ra, sa), y = host_frame(b, probe[f], rb, sb);
        if (x != y || memcmp(&sa, &sb, sizeof sa) || memcmp(ra.ics, rb.ics, sizeof ra.ics)) fail("state after the batch", it);
    }
    jaad_parser_destroy(a);
    jaad_parser_destroy(b);
}

static int copy_check()
{
    static const int lens[7] = {0, 1, 3, 4, 5, 8, 9};
    int bad = 0, n = 0;
    for (int phase = 0; phase < 8; phase++)
        for (int b0 = 0; b0 < 4; b0++)
            for (int li = 0; li < 7; li++)
                for (int pad = 0; pad < 6; pad += 5) {  // pad 0: the tail ends on the buffer's last byte
                    const int L = lens[li];
                    const size_t size = (size_t)b0 + L + pad;
                    uint8_t* d = (uint8_t*)malloc(size ? size : 1);
                    for (size_t i = 0; i < size; i++) d[i] = (uint8_t)rnd();
                    const uint64_t nbits = L ? (uint64_t)L * 8 - phase : 0, src_bit = (uint64_t)b0 * 8 + phase;
                    HostSrc src{d, size};
                    const uint32_t words = tail_pool_bytes((uint32_t)L) / 4 + 2;
                    for (uint32_t k = 0; k < words; k++) {
                        uint32_t want = 0;
                        for (uint32_t i = 0; i < 32; i++) {
                            const uint64_t t = 32ull * k + i, p = src_bit + t;
                            const uint32_t bit = t < nbits ? (d[p >> 3] >> (7 - (p & 7))) & 1u : 0u;
                            want = (want << 1) | bit;
                        }
                        if (tail_dword(src, src_bit, nbits, k) != want) bad++;
                        n++;
                    }
                    free(d);
                }
    printf("tail copy: %s (%d dwords)\n", bad ? "FAIL" : "ok", n);
    return bad;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int iters = atoi(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<Stream*> streams;
    unsigned char hdr[10];
    int last_run = -1;
    Stream* cur = nullptr;
    while (fread(hdr, 1, 10, f) == 10) {
        uint32_t n;
        memcpy(&n, hdr + 6, 4);
        std::vector<uint8_t> d(n);
        if (n && fread(d.data(), 1, n, f) != n) break;
        Stream* S = nullptr;
        for (Stream* k : streams)
            if (k->cfg.sf_index == hdr[0] && k->cfg.channel_config == hdr[1] && k->cfg.tns_mode == hdr[2] && k->cfg.ps == hdr[3] &&
                k->cfg.ext_sf_index == hdr[4] && k->run == hdr[5])
                S = k;
        if (!S) {
            S = new Stream;
            S->run = hdr[5];
            memset(&S->cfg, 0, sizeof S->cfg);
            S->cfg.abi_version = JAAD_ABI_VERSION;
            S->cfg.profile = 2;
            S->cfg.sf_index = hdr[0];
            S->cfg.channel_config = hdr[1];
            S->cfg.tns_mode = hdr[2];
            S->cfg.sbr = 1;
            S->cfg.ps = hdr[3];
            S->cfg.ext_sf_index = hdr[4];
            if (jaad_parser_create(&S->cfg, &S->H) || jaad_parser_create(&S->cfg, &S->S)) return 2;
            build_image(S->img, hdr[0], S->C);
            S->C.stereo = hdr[1] == 2;
            S->C.tns_spec = hdr[2] == JAAD_TNS_SPEC;
            streams.push_back(S);
        }
        if (S != cur || hdr[5] != last_run) S->runs.emplace_back();  // (one per Stream: a run id names a stream)
        cur = S;
        last_run = hdr[5];
        S->runs.back().push_back(d);
    }
    fclose(f);
    if (streams.empty()) return 2;
    int bad = copy_check();
    // every seed run as it is: all frames must parse, and some carry no payload
    int seeds_upsampled = 0;
    for (Stream* S : streams)
        for (size_t r = 0; r < S->runs.size(); r++) {
            if (both(*S, S->runs[r], -1, -1 - (int)r) != JAAD_OK) fail("seed status", -1 - (int)r);
            same_state(*S, S->runs[r], -1 - (int)r);
            jaad_parser* P = nullptr;
            if (jaad_parser_create(&S->cfg, &P)) return 2;
            static Rows rows;
            for (const std::vector<uint8_t>& fr : S->runs[r]) {
                jaad_sbr_frame rec;
                memset(&rec, 0, sizeof rec);
                if (host_frame(P, fr, rows, rec) == JAAD_OK && rec.status == JAAD_SBR_UPSAMPLE) seeds_upsampled++;
            }
            jaad_parser_destroy(P);
        }
    memset(counts, 0, sizeof counts);
    memset(tail_counts, 0, sizeof tail_counts);
    for (int it = 0; it < iters; it++) {
        Stream& S = *streams[rnd() % streams.size()];
        const std::vector<std::vector<uint8_t>>& run = S.runs[rnd() % S.runs.size()];
        // a window of up to four frames of the run, one of them mutated
        const size_t a = rnd() % run.size(), n = 1 + rnd() % (run.size() - a < 4 ? run.size() - a : 4);
        std::vector<std::vector<uint8_t>> w(run.begin() + a, run.begin() + a + n);
        const size_t m = rnd() % n;
        std::vector<uint8_t>& d = w[m];
        const int nflip = 1 + rnd() % 4;
        for (int j = 0; j < nflip; j++) {
            const size_t b = rnd() % (d.size() * 8);
            d[b >> 3] ^= (uint8_t)(0x80 >> (b & 7));
        }
        if (rnd() % 4 == 0) d.resize(rnd() % (d.size() + 1));
        both(S, w, (int)m, it);
        same_state(S, std::vector<std::vector<uint8_t>>(run.begin(), run.begin() + (run.size() < 2 ? run.size() : 2)), it);
    }
    for (Stream* S : streams) {
        jaad_parser_destroy(S->H);
        jaad_parser_destroy(S->S);
        delete S;
    }
    int total = 0;
    for (int i = 0; i < 16; i++) {
        if (counts[i]) printf("status %d: %d, in the tail %d\n", -i, counts[i], tail_counts[i]);
        total += counts[i];
    }
    printf("mutants: %d\n", total);
    printf("seed frames without a payload: %d\n", seeds_upsampled);
    printf("mismatches: %d\n", fails);
    return fails || bad ? 1 : 0;
}
