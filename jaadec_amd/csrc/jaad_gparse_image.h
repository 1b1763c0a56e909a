// Host side of jaad_parse_core.h: the table image (layout there) built from the reference's
// codebooks by Lut::build's rule (jaad_parse.cpp) -- primary table over the first min(maxlen, 10)
// bits, one secondary table per prefix whose codewords are longer -- with each entry carrying the
// codeword's length and its values in place of the row index.
#pragma once
#include <vector>

#include "jaad_parse_core.h"
#include "tables/jaad_huffman_tables.inc"
#include "tables/jaad_tables.inc"

namespace jaad {
namespace pcore {

inline uint32_t image_values(const int* row, int book)
{
    if (book == kBookSf) return (uint32_t)row[2];
    if (book < 4) {
        uint32_t v = 0;
        for (int j = 0; j < 4; j++) v |= ((uint32_t)row[2 + j] & 15u) << (4 * j);
        return v;
    }
    return ((uint32_t)row[2] & 0xFFu) | (((uint32_t)row[3] & 0xFFu) << 8);
}

inline void image_book(std::vector<uint32_t>& img, int book, const int* rows, int nrows, int stride)
{
    int maxlen = 0;
    for (int i = 0; i < nrows; i++) maxlen = rows[i * stride] > maxlen ? rows[i * stride] : maxlen;
    const int pbits = maxlen < 10 ? maxlen : 10, sbits = maxlen - pbits;
    const size_t first = img.size();
    img[kImgBooks + book * 4] = (uint32_t)maxlen;
    img[kImgBooks + book * 4 + 1] = (uint32_t)pbits;
    img[kImgBooks + book * 4 + 2] = (uint32_t)first;
    img.resize(first + ((size_t)1 << pbits), kNoCode);
    for (int i = 0; i < nrows; i++) {
        const int len = rows[i * stride];
        const uint32_t cw = (uint32_t)rows[i * stride + 1];
        const uint32_t ent = ((uint32_t)len << 16) | image_values(rows + i * stride, book);
        if (len <= pbits) {
            const uint32_t lo = cw << (pbits - len), n = 1u << (pbits - len);
            for (uint32_t k = 0; k < n; k++) img[first + lo + k] = ent;
        } else {
            const uint32_t pre = cw >> (len - pbits);
            if (img[first + pre] == kNoCode) {
                img[first + pre] = 0x80000000u | (uint32_t)(img.size() - first);
                img.resize(img.size() + ((size_t)1 << sbits), kNoCode);
            }
            const uint32_t base = img[first + pre] & 0x7FFFFFFFu;
            const int rest = len - pbits;
            const uint32_t lo = (cw & ((1u << rest) - 1u)) << (sbits - rest), n = 1u << (sbits - rest);
            for (uint32_t k = 0; k < n; k++) img[first + base + lo + k] = ent;
        }
    }
}

// the image for one sample-rate index (0..11); fills the band counts of C and points C.img at it
inline void build_image(std::vector<uint32_t>& img, int sf_index, Cfg& C)
{
    img.assign(kImgEntries, 0u);
    const int* r[11] = {&JAAD_HCB1[0][0], &JAAD_HCB2[0][0], &JAAD_HCB3[0][0], &JAAD_HCB4[0][0], &JAAD_HCB5[0][0],
                        &JAAD_HCB6[0][0], &JAAD_HCB7[0][0], &JAAD_HCB8[0][0], &JAAD_HCB9[0][0], &JAAD_HCB10[0][0],
                        &JAAD_HCB11[0][0]};
    const int n[11] = {81, 81, 81, 81, 81, 81, 64, 64, 169, 169, 289};
    for (int b = 0; b < 11; b++) image_book(img, b, r[b], n[b], b < 4 ? 6 : 4);
    image_book(img, kBookSf, &JAAD_HCB_SF[0][0], 121, 3);
    C.nswb_l = JAAD_SWB_LONG_WINDOW_COUNT[sf_index];
    C.nswb_s = JAAD_SWB_SHORT_WINDOW_COUNT[sf_index];
    for (int i = 0; i < 52; i++) img[kImgSwbLong + i] = i <= C.nswb_l ? (uint32_t)JAAD_SWB_OFFSET_LONG_WINDOW[sf_index][i] : 1024u;
    for (int i = 0; i < 16; i++) img[kImgSwbShort + i] = i <= C.nswb_s ? (uint32_t)JAAD_SWB_OFFSET_SHORT_WINDOW[sf_index][i] : 128u;
    lcg_pow_table(&img[kImgLcg]);
    C.img = img.data();
}

}  // namespace pcore
}  // namespace jaad
