// Device bitstream front end (include/jaad_gparse.h): AAC-LC raw_data_blocks in device memory ->
// the jaad_gpu.h batch records, by the parse code the host shares (jaad_parse_core.h).
//
//   gparse_frames_kernel  one lane per frame (a CPE's right channel starts where the left one
//                         ends, so a frame is the finest split).  The table image sits in LDS, with
//                         a 256-byte cb/sf work row per lane; bitstream reads go through a buffer
//                         resource over the caller's data buffer, so a read past it returns 0.
//   gparse_link_kernel    one wave per run: scans the LCG maps and the window shapes the frames
//                         left along the run and fills jaad_ics_info.pns_state / window_shape_prev.
// SBR configurations (jaad_gparse_batch_sbr): the frame kernel's SBR instantiation stops at a frame's
// first SBR fill element and reports where; then
//   gparse_tail_scan_kernel    one workgroup: exclusive scan of the tails' sizes -> pool offsets
//   gparse_tail_gather_kernel  one lane per 8 bytes of the pool: the tails, shifted to bit 0
// and the pool goes to the host, whose parser walks it (jaad_parse_tail.cpp).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/jaad_gparse.h"
#include "jaad_gparse_image.h"
#include "jaad_host_threads.h"
#include "jaad_parse_tail.h"

using namespace jaad::pcore;

namespace {

// Waves per workgroup.  The table image is 65.4 KiB of LDS and a wave's work rows 16.25 KiB, so a CU
// (160 KiB) holds one image: what shares it decides how many waves a CU runs.  Four waves (130.4
// KiB) put one wave on each SIMD, and a 65 536-frame batch is then 256 workgroups, one per CU.
#ifndef JAAD_GPARSE_WAVES
#define JAAD_GPARSE_WAVES 4
#endif
constexpr int kFrameLanes = 64 * JAAD_GPARSE_WAVES;
constexpr int kWorkStride = 260; // bytes of LDS per lane: cb[128], sf[128]; 65 dwords, so lanes
                                 // reading the same band hit different banks

// The frame's bytes in the data buffer.  Loads are aligned dwords through the buffer resource
// (num_records = the buffer's byte length: a dword wholly past it reads 0 without touching memory);
// the buffer's last, partial dword goes byte by byte, since a raw buffer load that straddles
// num_records returns 0 for all of it.
struct DevSrc {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t base, nbytes;
    __device__ uint32_t dword_be(uint32_t off) const
    {
        if (off + 4u <= nbytes || off >= nbytes)
            return __builtin_bswap32((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)off, 0, 0));
        uint32_t w = 0;
        for (uint32_t i = 0; i < 4; i++)
            w = (w << 8) | (uint32_t)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rsrc, (int)(off + i), 0, 0);
        return w;
    }
    __device__ uint64_t be64(uint64_t byte) const
    {
        const uint32_t at = base + (uint32_t)byte, al = at & ~3u, sh = (at & 3u) * 8u;
        const uint64_t w = ((uint64_t)dword_be(al) << 32) | dword_be(al + 4u);
        return sh ? (w << sh) | (dword_be(al + 8u) >> (32u - sh)) : w;
    }
};

struct FrameArgs {
    const uint8_t* data;
    uint32_t data_bytes, n_frames;
    const uint64_t* frame_off;
    const uint32_t* frame_len;
    int16_t* q;
    uint8_t *sf, *cb;
    jaad_ics_info* ics;
    uint64_t* ms;
    jaad_tns* tns;
    int8_t* status;
    uint32_t* link;
    const uint32_t* img;
    uint32_t img_words;
    int nswb_l, nswb_s, stereo, tns_spec;
};

struct DevOut {
    uint32_t* work;  // this lane's LDS row, zero between channels
    int16_t* q0;
    uint8_t *sf0, *cb0;
    jaad_tns* tns0;
    __device__ uint8_t* cb(int) { return reinterpret_cast<uint8_t*>(work); }
    __device__ uint8_t* sf(int) { return reinterpret_cast<uint8_t*>(work) + 128; }
    __device__ int16_t* q(int c) { return q0 + c * 1024; }
    __device__ jaad_tns* tns(int c) { return tns0 ? tns0 + c : nullptr; }
    __device__ void done(int c)  // the channel's rows to memory, 16 bytes a store; the work row zero again
    {
        uint4* dc = reinterpret_cast<uint4*>(cb0 + c * 128);
        uint4* ds = reinterpret_cast<uint4*>(sf0 + c * 128);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            dc[i] = make_uint4(work[4 * i], work[4 * i + 1], work[4 * i + 2], work[4 * i + 3]);
            ds[i] = make_uint4(work[32 + 4 * i], work[33 + 4 * i], work[34 + 4 * i], work[35 + 4 * i]);
        }
#pragma unroll
        for (int i = 0; i < 64; i++) work[i] = 0u;
    }
};

// SBR configurations: where a frame's tail lies, for the gather kernel and the host
struct TailArgs {
    uint32_t* src;  // [n_frames] byte offset in the data buffer of the tail's first byte
    uint2* info;    // [n_frames] {bytes from there to the frame's end, the tail's bit phase in that byte};
                    // bytes = 0: no tail
};

extern __shared__ uint32_t g_lds[];

template <bool kSbr>
__global__ __launch_bounds__(kFrameLanes) void gparse_frames_kernel(const FrameArgs A, const TailArgs T)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < A.img_words; i += kFrameLanes) g_lds[i] = A.img[i];
    uint32_t* work = g_lds + A.img_words + tid * (kWorkStride / 4);
    for (int i = 0; i < 64; i++) work[i] = 0u;
    __syncthreads();
    const uint32_t f = blockIdx.x * kFrameLanes + tid;
    if (f >= A.n_frames) return;
    const int nch = A.stereo ? 2 : 1;
    const size_t cf = (size_t)f * nch;

    uint64_t off = A.frame_off[f];
    uint32_t len = A.frame_len[f];
    if (off >= A.data_bytes) {
        off = 0;
        len = 0;
    } else if (len > A.data_bytes - (uint32_t)off) {
        len = A.data_bytes - (uint32_t)off;
    }
    DevSrc src;
    src.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(A.data), (short)0, (int)A.data_bytes, 0x00020000);
    src.base = (uint32_t)off;
    src.nbytes = A.data_bytes;
    Bits<DevSrc> br(src, len);
    Cfg C;
    C.img = g_lds;
    C.nswb_l = A.nswb_l;
    C.nswb_s = A.nswb_s;
    C.stereo = A.stereo;
    C.tns_spec = A.tns_spec;
    DevOut out;
    out.work = work;
    out.q0 = A.q + cf * 1024;
    out.sf0 = A.sf + cf * 128;
    out.cb0 = A.cb + cf * 128;
    out.tns0 = A.tns ? A.tns + cf : nullptr;
    FrameInfo F;
    int st;
    if (kSbr) {
        int64_t tail_bit;
        st = parse_frame_sbr(br, C, out, F, tail_bit);
        const bool has = st == JAAD_OK && tail_bit >= 0;  // tail_bit < 8 * len: the FIL's bytes are there
        const uint32_t skip = has ? (uint32_t)(tail_bit >> 3) : 0u;
        T.src[f] = has ? (uint32_t)off + skip : 0u;
        T.info[f] = has ? make_uint2(len - skip, (uint32_t)(tail_bit & 7)) : make_uint2(0u, 0u);
    } else {
        st = parse_frame(br, C, out, F);
    }
    A.status[f] = (int8_t)st;
    const bool moves = st == JAAD_OK || st == JAAD_ERR_EOS;
    for (int c = 0; c < nch; c++) A.link[cf + c] = moves ? link_pack(F.ch[c]) : 0u;
    if (st != JAAD_OK) return;
    for (int c = 0; c < nch; c++) {  // window_shape_prev / pns_state: gparse_link_kernel
        const ChInfo& I = F.ch[c];
        const uint32_t w0 = (uint32_t)I.seq | ((uint32_t)I.shape << 8) | ((uint32_t)I.max_sfb << 24);
        const uint32_t w1 = (uint32_t)I.grouping | ((uint32_t)I.flags << 8);
        *reinterpret_cast<uint4*>(A.ics + cf + c) = make_uint4(w0, w1, 0u, 0u);
    }
    if (A.stereo) *reinterpret_cast<ulonglong2*>(A.ms + (size_t)f * 2) = make_ulonglong2(F.ms[0], F.ms[1]);
}

struct LinkArgs {
    const uint32_t* frame_begin;
    const int8_t* status;
    const uint32_t* link;
    jaad_ics_info* ics;
    jaad_gparse_state* state;
    const uint32_t* lcg;
    uint32_t nch;
};

__global__ __launch_bounds__(64) void gparse_link_kernel(const LinkArgs A)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x, nch = A.nch;
    const uint32_t i0 = A.frame_begin[r] * nch, i1 = A.frame_begin[r + 1] * nch;
    uint32_t pns = A.state[r].pns_state;
    uint32_t shape[2] = {A.state[r].window_shape[0] & 1u, A.state[r].window_shape[1] & 1u};
    const uint32_t ch = lane % nch;  // i0 and the chunk length are multiples of nch
    for (uint32_t base = i0; base < i1; base += 64) {
        const uint32_t i = base + lane;
        const bool in = i < i1;
        int st = JAAD_ERR_INVALID_ARG;
        uint32_t p = 0;
        if (in) {
            st = A.status[i / nch];
            if (st == JAAD_OK || st == JAAD_ERR_EOS) p = A.link[i];
        }
        // inclusive scan of the LCG maps: lane l holds the steps of channel-frames base .. base + l
        Affine m = lcg_jump(A.lcg, link_steps(p));
        for (uint32_t d = 1; d < 64; d <<= 1) {
            Affine o = {__shfl_up(m.a, d), __shfl_up(m.c, d)};
            if (lane >= d) m = affine_then(o, m);
        }
        Affine ex = {__shfl_up(m.a, 1u), __shfl_up(m.c, 1u)};
        if (lane == 0) ex = affine_id();
        const uint32_t my_pns = affine_apply(ex, pns);
        // last valid shape per channel (lanes of one channel are nch apart)
        uint32_t v = link_shape(p);
        for (uint32_t d = nch; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(v, d);
            if (lane >= d && !(v & 2u)) v = o;
        }
        const uint32_t e = __shfl_up(v, nch);
        const uint32_t prev = (lane < nch || !(e & 2u)) ? shape[ch] : (e & 1u);
        if (in && st == JAAD_OK) {
            A.ics[i].window_shape_prev = (uint8_t)prev;
            A.ics[i].pns_state = my_pns;
        }
        Affine all = {__shfl(m.a, 63), __shfl(m.c, 63)};
        pns = affine_apply(all, pns);
        for (uint32_t c = 0; c < nch; c++) {
            const uint32_t t = __shfl(v, (int)(64 - nch + c));
            if (t & 2u) shape[c] = t & 1u;
        }
    }
    if (lane == 0) {
        A.state[r].pns_state = pns;
        A.state[r].window_shape[0] = (uint8_t)shape[0];
        if (nch == 2) A.state[r].window_shape[1] = (uint8_t)shape[1];
    }
}

// ---- the tail pool (SBR configurations) --------------------------------------------------------
// Each frame's tail -- its bits from the first SBR fill element after the channel element to its
// end -- goes, shifted to bit 0, into a dense pool the host parses from: tail f at pool_off[f],
// tail_pool_bytes(its bytes) long, zero from the frame's end on; 8 zero bytes end the pool.
constexpr int kScanLanes = 1024;

struct ScanArgs {
    const uint2* info;
    uint32_t* pool_off;  // [n_frames + 1]
    uint64_t* total;     // the pool's bytes before its padding (pool_off holds them mod 2^32)
    uint32_t n_frames;
};

// exclusive scan of the tails' pool sizes: one workgroup, a chunk of kScanLanes frames a step
__global__ __launch_bounds__(kScanLanes) void gparse_tail_scan_kernel(const ScanArgs A)
{
    __shared__ uint64_t wave_sum[kScanLanes / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < A.n_frames; base += kScanLanes) {
        const uint32_t f = base + tid;
        const uint64_t v = f < A.n_frames ? tail_pool_bytes(A.info[f].x) : 0u;
        uint64_t s = v;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_up(s, d);
            if (lane >= d) s += o;
        }
        if (lane == 63) wave_sum[wave] = s;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < kScanLanes / 64; w++) {
            if (w < wave) before += wave_sum[w];
            carry += wave_sum[w];
        }
        if (f < A.n_frames) A.pool_off[f] = (uint32_t)(before + s - v);
        __syncthreads();
    }
    if (tid == 0) {
        A.pool_off[A.n_frames] = (uint32_t)carry;
        A.total[0] = carry;
    }
}

struct GatherArgs {
    const uint8_t* data;
    uint32_t data_bytes, n_frames;
    const uint32_t* src;
    const uint2* info;
    const uint32_t* pool_off;
    uint2* pool;     // [units + 1]
    uint32_t units;  // the pool's 8-byte units before its padding (pool_off[n_frames] / 8, at least 1 frame)
};

// one lane per 8 bytes of the pool: finds its frame in pool_off and copies two dwords of its tail
__global__ __launch_bounds__(256) void gparse_tail_gather_kernel(const GatherArgs A)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u > A.units) return;
    uint32_t w0 = 0u, w1 = 0u;  // unit A.units is the padding
    if (u < A.units) {
        const uint32_t at = u * 8u;
        uint32_t lo = 0u, hi = A.n_frames;  // pool_off[lo] <= at < pool_off[hi]: the last such lo has bytes there
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (A.pool_off[mid] <= at)
                lo = mid;
            else
                hi = mid;
        }
        const uint2 in = A.info[lo];
        DevSrc src;
        src.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(A.data), (short)0, (int)A.data_bytes, 0x00020000);
        src.base = 0u;
        src.nbytes = A.data_bytes;
        const uint64_t src_bit = (uint64_t)A.src[lo] * 8u + in.y, nbits = (uint64_t)in.x * 8u - in.y;
        const uint64_t k = (at - A.pool_off[lo]) / 4u;
        w0 = tail_dword(src, src_bit, nbits, k);
        w1 = tail_dword(src, src_bit, nbits, k + 1u);
    }
    A.pool[u] = make_uint2(__builtin_bswap32(w0), __builtin_bswap32(w1));
}

}  // namespace

struct jaad_gparse {
    jaad_stream_cfg cfg{};
    int device = 0, nch = 1;
    Cfg C{};
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed = false;
    uint32_t* d_img = nullptr;
    uint32_t img_words = 0;
    size_t lds_bytes = 0;
    int8_t* d_status = nullptr;
    uint32_t* d_link = nullptr;
    size_t cap_frames = 0;
    uint32_t* d_fb = nullptr;
    jaad_gparse_state* d_state = nullptr;
    size_t cap_runs = 0;
    std::vector<jaad_gparse_state> h_state;
    // jaad_gparse_create_sbr: the tail path
    bool sbr = false;
    hipEvent_t ev_sbr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float ms_sbr[6] = {0, 0, 0, 0, 0, 0};
    bool timed_sbr = false;
    uint32_t* d_tsrc = nullptr;  // [cap_frames]
    // what goes back to the host after the link kernel, one block: total (8 bytes) | tail info
    // [frames][2] | state [runs] | pool_off [frames + 1] | status [frames]
    uint8_t* d_ret = nullptr;
    uint8_t* h_ret = nullptr;  // page-locked
    size_t cap_ret = 0;
    uint8_t *d_pool = nullptr, *h_pool = nullptr;  // h_pool page-locked
    size_t cap_pool = 0;
};

namespace {

int create(const jaad_stream_cfg* cfg, int device, jaad_gparse** out, bool sbr)
{
    if (!cfg || !out) return JAAD_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->abi_version != JAAD_ABI_VERSION) return JAAD_ERR_ABI;
    if (cfg->profile != 2 || cfg->sf_index > 11) return JAAD_ERR_UNSUPPORTED;
    if (!sbr && (cfg->sbr || cfg->ps)) return JAAD_ERR_UNSUPPORTED;  // SBR / PS payloads: jaad_gparse_create_sbr
    if (sbr && (!cfg->sbr || (cfg->ps && cfg->channel_config != 1))) return JAAD_ERR_UNSUPPORTED;
    if (cfg->channel_config < 1 || cfg->channel_config > 2) return JAAD_ERR_UNSUPPORTED;  // 3..7: the host parser
    if (cfg->tns_mode > JAAD_TNS_SPEC) return JAAD_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return JAAD_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return JAAD_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return JAAD_ERR_NO_DEVICE;
    jaad_gparse* gp = new (std::nothrow) jaad_gparse();
    if (!gp) return JAAD_ERR_NOMEM;
    gp->cfg = *cfg;
    gp->sbr = sbr;
    gp->device = device;
    gp->nch = cfg->channel_config == 2 ? 2 : 1;
    std::vector<uint32_t> img;
    build_image(img, cfg->sf_index, gp->C);
    gp->C.img = nullptr;
    gp->C.stereo = gp->nch == 2;
    gp->C.tns_spec = cfg->tns_mode == JAAD_TNS_SPEC;
    gp->img_words = (uint32_t)img.size();
    gp->lds_bytes = img.size() * 4 + (size_t)kFrameLanes * kWorkStride;
    auto bail = [&](hipError_t e, const char* what) {
        std::fprintf(stderr, "jaad_gparse_create: %s: %s\n", what, hipGetErrorString(e));
        jaad_gparse_destroy(gp);
        return JAAD_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&gp->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    for (int i = 0; i < 4; i++)
        if ((e = hipEventCreate(&gp->ev[i])) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipMalloc(&gp->d_img, img.size() * 4)) != hipSuccess) return bail(e, "hipMalloc tables");
    if ((e = hipMemcpy(gp->d_img, img.data(), img.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy tables");
    const void* kernel = sbr ? reinterpret_cast<const void*>(gparse_frames_kernel<true>)
                             : reinterpret_cast<const void*>(gparse_frames_kernel<false>);
    if ((e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gp->lds_bytes)) != hipSuccess)
        return bail(e, "hipFuncSetAttribute");
    if (sbr)
        for (int i = 0; i < 8; i++)
            if ((e = hipEventCreate(&gp->ev_sbr[i])) != hipSuccess) return bail(e, "hipEventCreate");
    *out = gp;
    return JAAD_OK;
}

// the size checks both batch entries make on the host before any launch
int check_sizes(const jaad_gparse* gp, const jaad_gparse_in* in, const jaad_gparse_out* out)
{
    const uint32_t nf = in->n_frames, nr = in->n_runs, nch = (uint32_t)gp->nch;
    if (!nf || !nr || !in->frame_begin || !in->data || !in->frame_off || !in->frame_len) return JAAD_ERR_INVALID_ARG;
    if (nf > 0x7FFFFFFFu / nch) return JAAD_ERR_INVALID_ARG;
    if (in->frame_begin[0] != 0 || in->frame_begin[nr] != nf) return JAAD_ERR_INVALID_ARG;
    for (uint32_t r = 0; r < nr; r++)
        if (in->frame_begin[r] > in->frame_begin[r + 1]) return JAAD_ERR_INVALID_ARG;
    if (!in->data_bytes || in->data_bytes >= 0xFFFFFFF0ull || ((uintptr_t)in->data & 3u)) return JAAD_ERR_INVALID_ARG;
    if (!out->q || !out->sf || !out->cb || !out->ics || (nch == 2 && !out->ms_used)) return JAAD_ERR_INVALID_ARG;
    if (((uintptr_t)out->q | (uintptr_t)out->sf | (uintptr_t)out->cb | (uintptr_t)out->ics | (uintptr_t)out->ms_used) & 15u)
        return JAAD_ERR_INVALID_ARG;
    if (((uintptr_t)in->frame_off & 7u) || ((uintptr_t)in->frame_len & 3u) || ((uintptr_t)out->tns & 3u)) return JAAD_ERR_INVALID_ARG;
    return JAAD_OK;
}

FrameArgs frame_args(const jaad_gparse* gp, const jaad_gparse_in* in, const jaad_gparse_out* out, int8_t* status)
{
    FrameArgs fa;
    fa.data = in->data;
    fa.data_bytes = (uint32_t)in->data_bytes;
    fa.n_frames = in->n_frames;
    fa.frame_off = in->frame_off;
    fa.frame_len = in->frame_len;
    fa.q = out->q;
    fa.sf = out->sf;
    fa.cb = out->cb;
    fa.ics = out->ics;
    fa.ms = out->ms_used;
    fa.tns = out->tns;
    fa.status = status;
    fa.link = gp->d_link;
    fa.img = gp->d_img;
    fa.img_words = gp->img_words;
    fa.nswb_l = gp->C.nswb_l;
    fa.nswb_s = gp->C.nswb_s;
    fa.stereo = gp->C.stereo;
    fa.tns_spec = gp->C.tns_spec;
    return fa;
}

}  // namespace

extern "C" {

int jaad_gparse_create(const jaad_stream_cfg* cfg, int device, jaad_gparse** out) { return create(cfg, device, out, false); }
int jaad_gparse_create_sbr(const jaad_stream_cfg* cfg, int device, jaad_gparse** out) { return create(cfg, device, out, true); }

void jaad_gparse_destroy(jaad_gparse* gp)
{
    if (!gp) return;
    (void)hipSetDevice(gp->device);
    if (gp->stream) (void)hipStreamSynchronize(gp->stream);
    for (void* p : {(void*)gp->d_img, (void*)gp->d_status, (void*)gp->d_link, (void*)gp->d_fb, (void*)gp->d_state,
                    (void*)gp->d_tsrc, (void*)gp->d_ret, (void*)gp->d_pool})
        if (p) (void)hipFree(p);
    if (gp->h_ret) (void)hipHostFree(gp->h_ret);
    if (gp->h_pool) (void)hipHostFree(gp->h_pool);
    for (int i = 0; i < 4; i++)
        if (gp->ev[i]) (void)hipEventDestroy(gp->ev[i]);
    for (int i = 0; i < 8; i++)
        if (gp->ev_sbr[i]) (void)hipEventDestroy(gp->ev_sbr[i]);
    if (gp->stream) (void)hipStreamDestroy(gp->stream);
    delete gp;
}

int jaad_gparse_batch(jaad_gparse* gp, const jaad_gparse_in* in, const jaad_gparse_out* out, int8_t* frame_result,
                      void* hip_stream)
{
    if (!gp || !in || !out || !frame_result) return JAAD_ERR_INVALID_ARG;
    if (gp->sbr) return JAAD_ERR_INVALID_ARG;  // jaad_gparse_batch_sbr
    const uint32_t nf = in->n_frames, nr = in->n_runs, nch = (uint32_t)gp->nch;
    if (!in->state || check_sizes(gp, in, out)) return JAAD_ERR_INVALID_ARG;

    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : gp->stream;
    hipError_t e = hipSuccess;
    auto hip = [&](hipError_t r, const char* what) {
        if (r != hipSuccess && e == hipSuccess) {
            e = r;
            std::fprintf(stderr, "jaad_gparse_batch: %s: %s\n", what, hipGetErrorString(r));
        }
        return r == hipSuccess;
    };
    if (!hip(hipSetDevice(gp->device), "hipSetDevice")) return JAAD_ERR_HIP;
    if (nf > gp->cap_frames) {
        (void)hipStreamSynchronize(s);
        if (gp->d_status) (void)hipFree(gp->d_status);
        if (gp->d_link) (void)hipFree(gp->d_link);
        gp->d_status = nullptr;
        gp->d_link = nullptr;
        gp->cap_frames = 0;
        if (!hip(hipMalloc(&gp->d_status, nf), "hipMalloc") || !hip(hipMalloc(&gp->d_link, (size_t)nf * nch * 4), "hipMalloc"))
            return JAAD_ERR_HIP;
        gp->cap_frames = nf;
    }
    if (nr > gp->cap_runs) {
        (void)hipStreamSynchronize(s);
        if (gp->d_fb) (void)hipFree(gp->d_fb);
        if (gp->d_state) (void)hipFree(gp->d_state);
        gp->d_fb = nullptr;
        gp->d_state = nullptr;
        gp->cap_runs = 0;
        if (!hip(hipMalloc(&gp->d_fb, ((size_t)nr + 1) * 4), "hipMalloc") ||
            !hip(hipMalloc(&gp->d_state, (size_t)nr * sizeof(jaad_gparse_state)), "hipMalloc"))
            return JAAD_ERR_HIP;
        gp->cap_runs = nr;
    }
    const size_t ncf = (size_t)nf * nch;
    hip(hipMemcpyAsync(gp->d_fb, in->frame_begin, ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, s), "copy frame_begin");
    hip(hipMemcpyAsync(gp->d_state, in->state, (size_t)nr * sizeof(jaad_gparse_state), hipMemcpyHostToDevice, s), "copy state");
    hip(hipEventRecord(gp->ev[0], s), "hipEventRecord");
    // the core stores coded values only: the rows start out zero
    hip(hipMemsetAsync(out->q, 0, ncf * 2048, s), "zero q");
    if (out->tns) hip(hipMemsetAsync(out->tns, 0, ncf * sizeof(jaad_tns), s), "zero tns");
    hip(hipEventRecord(gp->ev[1], s), "hipEventRecord");
    if (e != hipSuccess) return JAAD_ERR_HIP;
    const FrameArgs fa = frame_args(gp, in, out, gp->d_status);
    hipLaunchKernelGGL(gparse_frames_kernel<false>, dim3((nf + kFrameLanes - 1) / kFrameLanes), dim3(kFrameLanes), gp->lds_bytes, s,
                       fa, TailArgs{nullptr, nullptr});
    hip(hipGetLastError(), "gparse_frames_kernel");
    hip(hipEventRecord(gp->ev[2], s), "hipEventRecord");
    LinkArgs la;
    la.frame_begin = gp->d_fb;
    la.status = gp->d_status;
    la.link = gp->d_link;
    la.ics = out->ics;
    la.state = gp->d_state;
    la.lcg = gp->d_img + kImgLcg;
    la.nch = nch;
    hipLaunchKernelGGL(gparse_link_kernel, dim3(nr), dim3(64), 0, s, la);
    hip(hipGetLastError(), "gparse_link_kernel");
    hip(hipEventRecord(gp->ev[3], s), "hipEventRecord");
    gp->h_state.resize(nr);
    hip(hipMemcpyAsync(frame_result, gp->d_status, nf, hipMemcpyDeviceToHost, s), "copy statuses");
    hip(hipMemcpyAsync(gp->h_state.data(), gp->d_state, (size_t)nr * sizeof(jaad_gparse_state), hipMemcpyDeviceToHost, s), "copy state");
    hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (e != hipSuccess) return JAAD_ERR_HIP;
    gp->timed = true;
    for (uint32_t f = 0; f < nf; f++)
        if (frame_result[f] != JAAD_OK && frame_result[f] != JAAD_ERR_EOS) return frame_result[f];
    std::memcpy(in->state, gp->h_state.data(), (size_t)nr * sizeof(jaad_gparse_state));
    return JAAD_OK;
}

int jaad_gparse_last_ms(jaad_gparse* gp, float ms[3])
{
    if (!gp || !ms || !gp->timed) return JAAD_ERR_INVALID_ARG;
    for (int i = 0; i < 3; i++)
        if (hipEventElapsedTime(&ms[i], gp->ev[i], gp->ev[i + 1]) != hipSuccess) return JAAD_ERR_HIP;
    return JAAD_OK;
}

int jaad_gparse_batch_sbr(jaad_gparse* gp, const jaad_gparse_in* in, const jaad_gparse_out* out, jaad_parser* const* parsers,
                          jaad_sbr_frame* sbr, int8_t* frame_result, void* hip_stream)
{
    using namespace jaad::parse;
    if (!gp || !in || !out || !parsers || !sbr || !frame_result) return JAAD_ERR_INVALID_ARG;
    if (!gp->sbr) return JAAD_ERR_INVALID_ARG;  // jaad_gparse_batch
    if (check_sizes(gp, in, out)) return JAAD_ERR_INVALID_ARG;
    const uint32_t nf = in->n_frames, nr = in->n_runs, nch = (uint32_t)gp->nch;
    for (uint32_t r = 0; r < nr; r++)
        if (!parsers[r] || std::memcmp(&parser_cfg(parsers[r]), &gp->cfg, sizeof gp->cfg) != 0) return JAAD_ERR_INVALID_ARG;

    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : gp->stream;
    hipError_t e = hipSuccess;
    auto hip = [&](hipError_t r, const char* what) {
        if (r != hipSuccess && e == hipSuccess) {
            e = r;
            std::fprintf(stderr, "jaad_gparse_batch_sbr: %s: %s\n", what, hipGetErrorString(r));
        }
        return r == hipSuccess;
    };
    if (!hip(hipSetDevice(gp->device), "hipSetDevice")) return JAAD_ERR_HIP;
    if (nf > gp->cap_frames) {
        (void)hipStreamSynchronize(s);
        if (gp->d_link) (void)hipFree(gp->d_link);
        if (gp->d_tsrc) (void)hipFree(gp->d_tsrc);
        gp->d_link = nullptr;
        gp->d_tsrc = nullptr;
        gp->cap_frames = 0;
        if (!hip(hipMalloc(&gp->d_link, (size_t)nf * nch * 4), "hipMalloc") || !hip(hipMalloc(&gp->d_tsrc, (size_t)nf * 4), "hipMalloc"))
            return JAAD_ERR_HIP;
        gp->cap_frames = nf;
    }
    if (nr > gp->cap_runs) {
        (void)hipStreamSynchronize(s);
        if (gp->d_fb) (void)hipFree(gp->d_fb);
        gp->d_fb = nullptr;
        gp->cap_runs = 0;
        if (!hip(hipMalloc(&gp->d_fb, ((size_t)nr + 1) * 4), "hipMalloc")) return JAAD_ERR_HIP;
        gp->cap_runs = nr;
    }
    // the block that goes back after the link kernel
    const size_t o_info = 8, o_state = o_info + (size_t)nf * 8, o_off = o_state + (size_t)nr * sizeof(jaad_gparse_state),
                 o_status = o_off + ((size_t)nf + 1) * 4, ret_bytes = o_status + nf;
    auto ensure = [&](uint8_t*& d, uint8_t*& h, size_t& cap, size_t n) {
        if (n <= cap) return true;
        (void)hipStreamSynchronize(s);
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        cap = 0;
        const size_t want = n + n / 2;
        if (!hip(hipMalloc(&d, want), "hipMalloc") || !hip(hipHostMalloc(&h, want, hipHostMallocDefault), "hipHostMalloc")) return false;
        cap = want;
        return true;
    };
    if (!ensure(gp->d_ret, gp->h_ret, gp->cap_ret, ret_bytes)) return JAAD_ERR_HIP;
    if (!ensure(gp->d_pool, gp->h_pool, gp->cap_pool, 8)) return JAAD_ERR_HIP;
    jaad_gparse_state* h_state = reinterpret_cast<jaad_gparse_state*>(gp->h_ret + o_state);
    for (uint32_t r = 0; r < nr; r++) {
        std::memset(&h_state[r], 0, sizeof h_state[r]);
        parser_core_state(parsers[r], h_state[r].pns_state, h_state[r].window_shape);
    }
    uint2* d_info = reinterpret_cast<uint2*>(gp->d_ret + o_info);
    jaad_gparse_state* d_state = reinterpret_cast<jaad_gparse_state*>(gp->d_ret + o_state);
    uint32_t* d_off = reinterpret_cast<uint32_t*>(gp->d_ret + o_off);
    int8_t* d_status = reinterpret_cast<int8_t*>(gp->d_ret + o_status);
    hipEvent_t* ev = gp->ev_sbr;
    const size_t ncf = (size_t)nf * nch;
    hip(hipMemcpyAsync(gp->d_fb, in->frame_begin, ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, s), "copy frame_begin");
    hip(hipMemcpyAsync(d_state, h_state, (size_t)nr * sizeof(jaad_gparse_state), hipMemcpyHostToDevice, s), "copy state");
    hip(hipEventRecord(ev[0], s), "hipEventRecord");
    hip(hipMemsetAsync(out->q, 0, ncf * 2048, s), "zero q");
    if (out->tns) hip(hipMemsetAsync(out->tns, 0, ncf * sizeof(jaad_tns), s), "zero tns");
    hip(hipEventRecord(ev[1], s), "hipEventRecord");
    if (e != hipSuccess) return JAAD_ERR_HIP;
    const FrameArgs fa = frame_args(gp, in, out, d_status);
    hipLaunchKernelGGL(gparse_frames_kernel<true>, dim3((nf + kFrameLanes - 1) / kFrameLanes), dim3(kFrameLanes), gp->lds_bytes, s,
                       fa, TailArgs{gp->d_tsrc, d_info});
    hip(hipGetLastError(), "gparse_frames_kernel");
    hip(hipEventRecord(ev[2], s), "hipEventRecord");
    LinkArgs la;
    la.frame_begin = gp->d_fb;
    la.status = d_status;
    la.link = gp->d_link;
    la.ics = out->ics;
    la.state = d_state;
    la.lcg = gp->d_img + kImgLcg;
    la.nch = nch;
    hipLaunchKernelGGL(gparse_link_kernel, dim3(nr), dim3(64), 0, s, la);
    hip(hipGetLastError(), "gparse_link_kernel");
    hip(hipEventRecord(ev[3], s), "hipEventRecord");
    ScanArgs sa;
    sa.info = d_info;
    sa.pool_off = d_off;
    sa.total = reinterpret_cast<uint64_t*>(gp->d_ret);
    sa.n_frames = nf;
    hipLaunchKernelGGL(gparse_tail_scan_kernel, dim3(1), dim3(kScanLanes), 0, s, sa);
    hip(hipGetLastError(), "gparse_tail_scan_kernel");
    hip(hipEventRecord(ev[4], s), "hipEventRecord");
    // first trip: the sizes (with the statuses and the runs' state)
    hip(hipMemcpyAsync(gp->h_ret, gp->d_ret, ret_bytes, hipMemcpyDeviceToHost, s), "copy sizes");
    hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (e != hipSuccess) return JAAD_ERR_HIP;
    uint64_t total;
    std::memcpy(&total, gp->h_ret, 8);
    if (total >= 0xFFFFFFF0ull) return JAAD_ERR_INVALID_ARG;  // overlapping frames: tails of 4 GiB together
    if (total) {
        if (!ensure(gp->d_pool, gp->h_pool, gp->cap_pool, (size_t)total + 8)) return JAAD_ERR_HIP;
        GatherArgs ga;
        ga.data = in->data;
        ga.data_bytes = (uint32_t)in->data_bytes;
        ga.n_frames = nf;
        ga.src = gp->d_tsrc;
        ga.info = d_info;
        ga.pool_off = d_off;
        ga.pool = reinterpret_cast<uint2*>(gp->d_pool);
        ga.units = (uint32_t)(total / 8);
        hip(hipEventRecord(ev[5], s), "hipEventRecord");
        hipLaunchKernelGGL(gparse_tail_gather_kernel, dim3(ga.units / 256u + 1u), dim3(256), 0, s, ga);
        hip(hipGetLastError(), "gparse_tail_gather_kernel");
        hip(hipEventRecord(ev[6], s), "hipEventRecord");
        // second trip: the pool
        hip(hipMemcpyAsync(gp->h_pool, gp->d_pool, (size_t)total + 8, hipMemcpyDeviceToHost, s), "copy pool");
        hip(hipEventRecord(ev[7], s), "hipEventRecord");
        hip(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (e != hipSuccess) return JAAD_ERR_HIP;
    } else {
        std::memset(gp->h_pool, 0, 8);
    }
    float* ms = gp->ms_sbr;
    float t = 0.0f;
    for (int i = 0; i < 4; i++) hip(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]), "hipEventElapsedTime");
    ms[4] = 0.0f;
    if (total) {
        hip(hipEventElapsedTime(&t, ev[5], ev[6]), "hipEventElapsedTime");
        ms[3] += t;
        hip(hipEventElapsedTime(&ms[4], ev[6], ev[7]), "hipEventElapsedTime");
    }
    if (e != hipSuccess) return JAAD_ERR_HIP;
    TailBatch tb;
    tb.n_frames = nf;
    tb.n_runs = nr;
    tb.frame_begin = in->frame_begin;
    tb.core_status = reinterpret_cast<const int8_t*>(gp->h_ret + o_status);
    tb.pool_off = reinterpret_cast<const uint32_t*>(gp->h_ret + o_off);
    tb.tail_info = reinterpret_cast<const uint32_t*>(gp->h_ret + o_info);
    tb.pool = gp->h_pool;
    tb.core_state = h_state;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = parse_tails(parsers, tb, sbr, frame_result, jaad::host_threads());
    ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    gp->timed_sbr = true;
    return rc;
}

int jaad_gparse_last_ms_sbr(jaad_gparse* gp, float ms[6])
{
    if (!gp || !ms || !gp->timed_sbr) return JAAD_ERR_INVALID_ARG;
    std::memcpy(ms, gp->ms_sbr, sizeof gp->ms_sbr);
    return JAAD_OK;
}

}  // extern "C"
