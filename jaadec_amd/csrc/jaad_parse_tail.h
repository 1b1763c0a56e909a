// The host half of a frame whose channel element was parsed on the device (include/jaad_gparse.h,
// jaad_gparse_batch_sbr): everything from the first SBR fill element after the channel element to
// the frame's end -- the tail -- goes through the host parser's own element loop (jaad_parse.cpp),
// with the SBR / PS history of the run's jaad_parser.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/jaad_gparse.h"
#include "../../include/jaad_parse.h"

namespace jaad {
namespace parse {

const jaad_stream_cfg& parser_cfg(const jaad_parser* p);
// the PNS LCG and the window shapes, the state the device's link pass carries
void parser_core_state(const jaad_parser* p, uint32_t& pns, uint8_t shape[2]);
void parser_set_core_state(jaad_parser* p, uint32_t pns, const uint8_t shape[2]);

// One frame of a mono / stereo SBR configuration whose core ended with core_status.  *rec is
// zeroed; a core status other than 0 is the frame's.  Otherwise the element loop of
// parse_frame_body runs over the tail -- `bits` bits at tail[0] bit 0, cut out of the frame at bit
// phase `phase` (mod 8), readable up to tail + phys_bytes; bits = 0: the frame had none -- as after
// the channel element, and then the checks that end a frame.  p's SBR / PS state moves as
// jaad_parse_frame moves it (status 0 or JAAD_ERR_EOS); the PNS LCG and the window shapes are the
// caller's (parser_set_core_state).  in_place: without the copy of the state that makes a refused
// frame leave it untouched (two copies of ~10 KB a frame) -- after a status other than 0 or
// JAAD_ERR_EOS p's state is void, and the caller starts over from a copy of its own.
int parse_tail_frame(jaad_parser* p, int core_status, const uint8_t* tail, size_t phys_bytes, size_t bits, unsigned phase,
                     jaad_sbr_frame* rec, bool in_place = false);

// What came back from the device for a batch (jaad_gparse.hip): per frame the core's status, its
// tail's offset in the pool (pool_off [n_frames + 1], multiples of 8) and {bytes, bit phase}
// (tail_info [n_frames][2], bytes = 0: no tail); the pool ends with 8 zero bytes.
struct TailBatch {
    uint32_t n_frames, n_runs;
    const uint32_t* frame_begin;
    const int8_t* core_status;
    const uint32_t* pool_off;
    const uint32_t* tail_info;
    const uint8_t* pool;
    const jaad_gparse_state* core_state;  // [n_runs] after the batch (the link pass)
};

// The tail stage of a batch: run r's frames in order on a copy of parsers[r], runs spread over
// `threads` threads.  sbr [n_frames] and frame_result [n_frames] are filled.  When every frame
// ends 0 or JAAD_ERR_EOS the copies (with core_state) are committed to parsers[] and the result is
// JAAD_OK; otherwise the first other status in frame order, parsers[] as they were.
int parse_tails(jaad_parser* const* parsers, const TailBatch& B, jaad_sbr_frame* sbr, int8_t* frame_result, int threads);

}  // namespace parse
}  // namespace jaad
