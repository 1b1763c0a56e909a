// Host tail stage of the device bitstream front end (jaad_parse_tail.h): per run, in frame order,
// the host parser's element loop over what the device left of each frame.
#include "jaad_parse_tail.h"

#include <atomic>
#include <thread>
#include <vector>

namespace jaad {
namespace parse {

int parse_tails(jaad_parser* const* parsers, const TailBatch& B, jaad_sbr_frame* sbr, int8_t* frame_result, int threads)
{
    const uint32_t nr = B.n_runs;
    std::vector<jaad_parser*> work(nr, nullptr);
    auto drop = [&] {
        for (jaad_parser* w : work) jaad_parser_destroy(w);
    };
    for (uint32_t r = 0; r < nr; r++)
        if (jaad_parser_clone(parsers[r], &work[r]) != JAAD_OK) {
            drop();
            return JAAD_ERR_NOMEM;
        }
    std::atomic<uint32_t> next{0};
    // One run.  in_place: the state moves without per-frame copies; false when a frame was refused,
    // after which the state is void and the run has to start over.
    auto run = [&](uint32_t r, bool in_place) {
        for (uint32_t f = B.frame_begin[r]; f < B.frame_begin[r + 1]; f++) {
            const uint32_t bytes = B.tail_info[2 * f], phase = B.tail_info[2 * f + 1];
            const uint32_t at = B.pool_off[f];
            // readable: the tail's own 8-byte units and at least the pool's 8 zero bytes after them
            const size_t phys = (((size_t)bytes + 7u) & ~(size_t)7u) + 8u;
            const int st = parse_tail_frame(work[r], B.core_status[f], B.pool + at, phys, bytes ? (size_t)bytes * 8u - phase : 0u,
                                            phase, &sbr[f], in_place);
            frame_result[f] = (int8_t)st;
            if (in_place && st != JAAD_OK && st != JAAD_ERR_EOS && B.core_status[f] == JAAD_OK) return false;
        }
        return true;
    };
    auto worker = [&] {
        for (uint32_t r; (r = next.fetch_add(1)) < nr;)
            if (!run(r, true)) {  // a refused frame: once more from the start, every frame on a copy of the state
                jaad_parser_copy(work[r], parsers[r]);
                run(r, false);
            }
    };
    const int nt = threads < 1 ? 1 : ((uint32_t)threads > nr ? (int)nr : threads);
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(worker);
    worker();
    for (std::thread& t : th) t.join();
    int rc = JAAD_OK;
    for (uint32_t f = 0; f < B.n_frames && !rc; f++)
        if (frame_result[f] != JAAD_OK && frame_result[f] != JAAD_ERR_EOS) rc = frame_result[f];
    if (!rc)
        for (uint32_t r = 0; r < nr; r++) {
            jaad_parser_copy(parsers[r], work[r]);
            parser_set_core_state(parsers[r], B.core_state[r].pns_state, B.core_state[r].window_shape);
        }
    drop();
    return rc;
}

}  // namespace parse
}  // namespace jaad
