// Differential check of the shared parse core (jaadec_amd/csrc/jaad_parse_core.h) against the host
// parser (jaad_parse_frame), built for the host with AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_gparse_core.py.  Seed frames (valid AAC-LC raw_data_blocks from the test writer)
// and bit-flipped / truncated mutants of them go through both: the core plus a scalar restatement
// of the link pass on one side, a jaad_parser with the same state on the other.  Required: the
// same status; for status 0 the same q / sf / cb / ics / ms_used / tns bytes; for 0 and EOS the
// same state afterwards (the PNS LCG directly, the window shapes through the records of the seed
// frame parsed next).  Also the LCG jump: n steps by the power table equal n single steps.
// Usage: gparse_diff <seeds.bin> <mutants>; seeds.bin: records of {u8 sf_index, u8 channel_config,
// u8 tns_mode, u32 bytes, bytes}.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jaad_gparse_image.h"
#include "jaad_parse.h"

using namespace jaad::pcore;

static uint64_t rs = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return (uint32_t)(rs >> 11);
}

struct HostSrc {
    const uint8_t* d;
    size_t n;
    uint64_t be64(uint64_t byte) const
    {
        uint64_t w = 0;
        for (size_t i = 0; i < 8; i++) w = (w << 8) | (byte + i < n ? d[byte + i] : 0u);
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

struct Stream {  // one configuration: the host parser and the core's side of the same state
    jaad_stream_cfg cfg;
    jaad_parser* P = nullptr;
    std::vector<uint32_t> img;
    Cfg C;
    uint32_t pns = 0x1F2E3D4Cu;
    int shape[2] = {0, 0};
};

static int fails = 0;
static void fail(const char* what, int it)
{
    if (fails++ < 20) fprintf(stderr, "MISMATCH %s (iteration %d)\n", what, it);
}

// one frame through both sides; returns the (common) status, or 1 when they differ
static int both(Stream& S, const uint8_t* data, size_t n, int it)
{
    const int nch = S.C.stereo ? 2 : 1;
    static Rows h, c;
    h.clear();
    c.clear();
    jaad_frame_out o;
    memset(&o, 0, sizeof o);
    o.q = h.q[0];
    o.sf = h.sf[0];
    o.cb = h.cb[0];
    o.ics = h.ics;
    o.ms_used = h.ms;
    o.tns = h.tns;
    const int sh = jaad_parse_frame(S.P, data, n, &o);
    RowsOut out{&c};
    FrameInfo F;
    HostSrc src{data, n};
    Bits<HostSrc> br(src, n);
    const int sc = parse_frame(br, S.C, out, F);
    if (sc != sh) {
        fprintf(stderr, "status: core %d host %d\n", sc, sh);
        fail("status", it);
        return 1;
    }
    if (sc != JAAD_OK && sc != JAAD_ERR_EOS) return sc;
    // the link pass, scalar: channels in order, each seeing the state before it
    for (int ch = 0; ch < nch; ch++) {
        const ChInfo& I = F.ch[ch];
        if (sc == JAAD_OK) {
            jaad_ics_info& ic = c.ics[ch];
            ic.window_sequence = I.seq;
            ic.window_shape = I.shape;
            ic.window_shape_prev = (uint8_t)S.shape[ch];
            ic.max_sfb = I.max_sfb;
            ic.grouping = I.grouping;
            ic.flags = I.flags;
            ic.pns_state = S.pns;
        }
        S.pns = affine_apply(lcg_jump(&S.img[kImgLcg], I.noise_steps), S.pns);
    }
    for (int ch = 0; ch < nch; ch++)
        if (F.ch[ch].shape_valid) S.shape[ch] = F.ch[ch].shape;
    c.ms[0] = F.ms[0];
    c.ms[1] = F.ms[1];
    if (S.pns != jaad_parser_pns_state(S.P)) fail("pns state after the frame", it);
    if (sc == JAAD_OK) {
        if (memcmp(h.q, c.q, sizeof(int16_t) * 1024 * nch)) fail("q", it);
        if (memcmp(h.sf, c.sf, sizeof h.sf)) fail("sf", it);
        if (memcmp(h.cb, c.cb, sizeof h.cb)) fail("cb", it);
        if (memcmp(h.ics, c.ics, sizeof(jaad_ics_info) * nch)) fail("ics", it);
        if (nch == 2 && memcmp(h.ms, c.ms, sizeof h.ms)) fail("ms_used", it);
        if (memcmp(h.tns, c.tns, sizeof(jaad_tns) * nch)) fail("tns", it);
    }
    return sc;
}

static int lcg_check()
{
    uint32_t t[64];
    lcg_pow_table(t);
    const uint32_t ns[8] = {0, 1, 2, 63, 64, 65, 1023, (1u << 20) + 7};
    int bad = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x = 0x1F2E3D4Cu;
        for (uint32_t k = 0; k < ns[i]; k++) x = 1664525u * x + 1013904223u;
        if (affine_apply(lcg_jump(t, ns[i]), 0x1F2E3D4Cu) != x) bad++;
        for (int j = 0; j < 8; j++) {  // two jumps compose to the jump of the sum
            const Affine m = affine_then(lcg_jump(t, ns[i]), lcg_jump(t, ns[j])), s = lcg_jump(t, ns[i] + ns[j]);
            if (m.a != s.a || m.c != s.c) bad++;
        }
    }
    printf("lcg jump: %s\n", bad ? "FAIL" : "ok");
    return bad;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int iters = atoi(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    struct Seed {
        int stream;
        std::vector<uint8_t> d;
    };
    std::vector<Seed> seeds;
    std::vector<Stream*> streams;
    unsigned char hdr[7];
    while (fread(hdr, 1, 7, f) == 7) {
        uint32_t n;
        memcpy(&n, hdr + 3, 4);
        Seed s;
        s.d.resize(n);
        if (n && fread(s.d.data(), 1, n, f) != n) break;
        s.stream = -1;
        for (size_t k = 0; k < streams.size(); k++)
            if (streams[k]->cfg.sf_index == hdr[0] && streams[k]->cfg.channel_config == hdr[1] && streams[k]->cfg.tns_mode == hdr[2])
                s.stream = (int)k;
        if (s.stream < 0) {
            Stream* S = new Stream;
            memset(&S->cfg, 0, sizeof S->cfg);
            S->cfg.abi_version = JAAD_ABI_VERSION;
            S->cfg.profile = 2;
            S->cfg.sf_index = hdr[0];
            S->cfg.channel_config = hdr[1];
            S->cfg.tns_mode = hdr[2];
            if (jaad_parser_create(&S->cfg, &S->P)) return 2;
            build_image(S->img, hdr[0], S->C);
            S->C.stereo = hdr[1] == 2;
            S->C.tns_spec = hdr[2] == JAAD_TNS_SPEC;
            s.stream = (int)streams.size();
            streams.push_back(S);
        }
        seeds.push_back(s);
    }
    fclose(f);
    if (seeds.empty()) return 2;
    int bad = lcg_check();
    int counts[16] = {0};
    // every seed as it is: all must parse
    for (size_t i = 0; i < seeds.size(); i++)
        if (both(*streams[seeds[i].stream], seeds[i].d.data(), seeds[i].d.size(), -1 - (int)i) != JAAD_OK) fail("seed status", -1 - (int)i);
    for (int it = 0; it < iters; it++) {
        const Seed& s = seeds[rnd() % seeds.size()];
        Stream& S = *streams[s.stream];
        std::vector<uint8_t> d = s.d;
        const int nflip = 1 + rnd() % 4;
        for (int j = 0; j < nflip; j++) {
            const size_t b = rnd() % (d.size() * 8);
            d[b >> 3] ^= (uint8_t)(0x80 >> (b & 7));
        }
        if (rnd() % 4 == 0) d.resize(rnd() % (d.size() + 1));
        // an exact-size heap copy: a read past the frame is an AddressSanitizer report
        uint8_t* data = d.empty() ? nullptr : (uint8_t*)malloc(d.size());
        if (data) memcpy(data, d.data(), d.size());
        const int st = both(S, data, d.size(), it);
        free(data);
        if (st <= 0) counts[-st < 16 ? -st : 15]++;
        // the state the mutant left, seen through a good frame's records (window_shape_prev, pns_state)
        if (both(S, s.d.data(), s.d.size(), it) != JAAD_OK) fail("seed after mutant", it);
    }
    for (size_t k = 0; k < streams.size(); k++) {
        jaad_parser_destroy(streams[k]->P);
        delete streams[k];
    }
    for (int i = 0; i < 16; i++)
        if (counts[i]) printf("status %d: %d\n", -i, counts[i]);
    printf("mismatches: %d\n", fails);
    return fails || bad ? 1 : 0;
}
