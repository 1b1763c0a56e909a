/*
 * jaad_gparse.h -- device-side bitstream front end: AAC-LC raw_data_blocks in device memory to
 * the jaad_gpu.h batch records in device memory, without the host Huffman decode.
 *
 * The host parser (jaad_parse.h) fills one frame at a time on a CPU core.  Per frame the AAC-LC
 * parse carries only two values across a frame boundary -- each channel's previous window shape
 * and the static PNS LCG (A/syntax/ICStream.java:26,247) -- and neither changes how a frame's bits
 * are read.  So one kernel parses every frame of every run in parallel (one lane per frame) and a
 * second, short one links the two carried values along each run.  Both run the same parse code as
 * the differential check against jaad_parse_frame (jaadec_amd/csrc/jaad_parse_core.h): the
 * records equal jaad_parse_frame's byte for byte, and so does each frame's status.
 *
 * AAC-LC with channel_config 1 or 2: jaad_gparse_create / jaad_gparse_batch.
 *
 * HE-AAC (SBR, and PS on a mono core) with channel_config 1 or 2: jaad_gparse_create_sbr /
 * jaad_gparse_batch_sbr.  A frame's parse is split.  The device takes the channel element, as
 * above, and stops at the first fill element after it that carries an SBR payload; the frame's
 * bits from there to its end -- its tail: fill / data-stream elements, the SBR / PS payload, the
 * END element -- are small and sequential along a stream, and the host parses them.  A scan and a
 * gather kernel pack all tails, each shifted to bit 0 of an 8-byte aligned slot, into one pool that
 * goes back to the host in one copy; there the host parser's own element loop (jaad_parse_frame's)
 * walks each run's tails in order with the SBR / PS history of that run's jaad_parser, and fills
 * the jaad_sbr_frame records jaad_decode_batch_device takes from host memory.
 *
 * Same library as jaad_gpu.h (libjaadgpu.so).
 */
#ifndef JAAD_GPARSE_H
#define JAAD_GPARSE_H

#include <stddef.h>
#include <stdint.h>

#include "jaad_gpu.h"
#include "jaad_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jaad_gparse jaad_gparse;

/* What a run carries from one call to the next (host memory, in/out): the parser state of
 * jaad_parse.h for such a stream. */
typedef struct jaad_gparse_state {
    uint32_t pns_state;      /* 0x1F2E3D4C for a fresh parser (jaad_parser_pns_state)           */
    uint8_t window_shape[2]; /* ICSInfo.windowShape[CURRENT] per channel, 0 for a fresh parser   */
    uint8_t reserved[2];
} jaad_gparse_state;

typedef struct jaad_gparse_in {
    uint32_t n_frames, n_runs;
    const uint32_t* frame_begin; /* host [n_runs+1], as jaad_batch.frame_begin                       */
    const uint8_t* data;         /* dev: the bytes the frames lie in (ADTS headers may stay in);
                                    4-byte aligned, less than 2^32 - 16 bytes                        */
    size_t data_bytes;
    const uint64_t* frame_off;   /* dev [n_frames] byte offset of each raw_data_block in data        */
    const uint32_t* frame_len;   /* dev [n_frames] its bytes; a frame that reaches past data_bytes is
                                    parsed as cut off there                                          */
    jaad_gparse_state* state;    /* host [n_runs]                                                    */
} jaad_gparse_in;

typedef struct jaad_gparse_out { /* all device memory, the jaad_batch layouts */
    int16_t* q;                  /* [ch-frame][1024], 8-byte aligned */
    uint8_t* sf;                 /* [ch-frame][128], 4-byte aligned  */
    uint8_t* cb;                 /* [ch-frame][128], 4-byte aligned  */
    jaad_ics_info* ics;          /* [ch-frame]                       */
    uint64_t* ms_used;           /* [frame][2], channel_config 2     */
    jaad_tns* tns;               /* [ch-frame], or NULL: TNS data is parsed and dropped */
} jaad_gparse_out;

/* AAC-LC, channel_config 1 or 2, sbr = 0; JAAD_ERR_UNSUPPORTED for SBR / PS and configurations
 * 3..7 (they stay on the host parser), decided before a device is looked for.  JAAD_ERR_ABI on a
 * wrong abi_version, JAAD_ERR_NO_DEVICE without a gfx950 device, as jaad_ctx_create. */
int jaad_gparse_create(const jaad_stream_cfg* cfg, int device, jaad_gparse** out);
void jaad_gparse_destroy(jaad_gparse* gp);

/* Parse a batch: both kernels are queued on hip_stream (a hipStream_t, NULL = the parser's own
 * stream), the per-frame statuses are copied back, and the call returns once they are on the
 * host.  The records stay in device memory, ordered on that stream for a jaad_decode_batch_device
 * queued on it next.
 * frame_result[f] (host [n_frames]) is what jaad_parse_frame returns for the frame: 0,
 * JAAD_ERR_EOS, JAAD_ERR_BITSTREAM or JAAD_ERR_UNSUPPORTED (an SBR fill payload, a CCE, gain
 * control, a predictor: as for the host parser without those outputs).
 * Returns JAAD_OK when every frame is 0 or JAAD_ERR_EOS, and state[] has advanced; the caller
 * turns JAAD_ERR_EOS into JAAD_FRAME_EOS entries of jaad_batch.frame_status (the records of such a
 * frame are unspecified, and not read by the decode).  Otherwise the first other status in frame
 * order, with state[] as it was and the records unspecified.
 * Sizes are checked on the host before any launch (JAAD_ERR_INVALID_ARG): zero frames or runs, a
 * frame_begin that does not start at 0, end at n_frames or is not monotone, a NULL array that is
 * needed (ms_used for channel_config 2), data misaligned or too long. */
int jaad_gparse_batch(jaad_gparse* gp, const jaad_gparse_in* in, const jaad_gparse_out* out, int8_t* frame_result,
                      void* hip_stream);

/* Device times of the last jaad_gparse_batch, in milliseconds (HIP events on its stream): ms[0]
 * zeroing the q / tns rows, ms[1] the frame kernel, ms[2] the link kernel.  For measurements
 * (tools/bench_gparse.py); JAAD_ERR_INVALID_ARG before the first batch. */
int jaad_gparse_last_ms(jaad_gparse* gp, float ms[3]);

/* An SBR configuration: sbr = 1 (ps = 1 only with channel_config 1), channel_config 1 or 2, any
 * ext_sf_index jaad_parser_create accepts.  JAAD_ERR_UNSUPPORTED for sbr = 0 (jaad_gparse_create)
 * and configurations 3..7, decided before a device is looked for; otherwise as jaad_gparse_create.
 * The object serves jaad_gparse_batch_sbr only, one made by jaad_gparse_create jaad_gparse_batch
 * only: the other entry returns JAAD_ERR_INVALID_ARG before any launch. */
int jaad_gparse_create_sbr(const jaad_stream_cfg* cfg, int device, jaad_gparse** out);

/* Parse a batch of an SBR configuration.  in / out as for jaad_gparse_batch; in->state is ignored:
 * the carried state is parsers[r] (host [n_runs], each created with the parser object's
 * configuration), run r's host parser.  Its PNS LCG and window shapes go in, and after a
 * successful call it is exactly where jaad_parse_frame over the run's frames would have left it
 * (LCG, shapes, SBR / PS history), so host and device parsing can alternate on a stream, and
 * jaad_parser_clone / jaad_parser_copy stay the rollback tools.
 * sbr (host [n_frames], out) gets each frame's jaad_sbr_frame: zero for a frame whose core did not
 * parse, JAAD_SBR_UPSAMPLE for one without a payload, a payload read whole before the bitstream
 * ended kept (jaad_parse.h).  frame_result[f] is what jaad_parse_frame returns for the frame with
 * this configuration and without coupling outputs.  The core records are in device memory, ordered
 * on the stream, as for jaad_gparse_batch; the call returns once sbr and frame_result are written.
 * Returns JAAD_OK when every frame is 0 or JAAD_ERR_EOS, the parsers advanced; otherwise the first
 * other status in frame order, every parser as it was.  JAAD_ERR_INVALID_ARG also when the tails
 * together reach 2^32 - 16 bytes (frames that overlap in data). */
int jaad_gparse_batch_sbr(jaad_gparse* gp, const jaad_gparse_in* in, const jaad_gparse_out* out, jaad_parser* const* parsers,
                          jaad_sbr_frame* sbr, int8_t* frame_result, void* hip_stream);

/* Times of the last jaad_gparse_batch_sbr in milliseconds: ms[0] zeroing the q / tns rows, ms[1]
 * the frame kernel, ms[2] the link kernel, ms[3] the scan and the gather kernel, ms[4] the copy of
 * the pool to the host (HIP events on the call's stream), ms[5] the host tail stage (wall clock).
 * JAAD_ERR_INVALID_ARG before the first such batch. */
int jaad_gparse_last_ms_sbr(jaad_gparse* gp, float ms[6]);

#ifdef __cplusplus
}
#endif
#endif /* JAAD_GPARSE_H */
