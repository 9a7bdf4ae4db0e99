/* tests/cpu_shim/batch_compress/launchers_host.c -- the launchers of csrc/lzs_batch_compress.c stated on the CPU, from their
 * contracts in csrc/lzs_hip_shim.h and on the oracle's match finder (lzs_oracle_search), serially; nothing here is transcribed
 * from the kernels.  TEST INFRASTRUCTURE ONLY (tests/test_batch_compress_host.py): with ../lzs_cpu_shim.c, which has every other
 * launcher, the product's unchanged host sources run under the address and undefined-behaviour sanitizers.  "Device" memory is
 * malloc'ed memory, so a table or a slot that is too small is a heap overflow the sanitizer sees; a block's input is read
 * through a copy of exactly its length, so a read before or behind the block is one too. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lzs_hip_shim.h"

unsigned lzs_oracle_search(const uint8_t *in, size_t n, size_t c, unsigned *best_off);

/* what the driver asks afterwards: launches of either kind, and segments compressed in the last compress launch */
unsigned g_bc_compress_launches, g_bc_stitch_launches, g_bc_second_passes;

/* MSB-first bits ORed in at bit `at` of dst, bytes at or past `limit` dropped */
static void or_bits(uint8_t *dst, uint64_t limit, uint64_t at, uint32_t value, unsigned width)
{
    for (unsigned i = 0; i < width; i++) {
        const uint64_t bit = at + i;
        if (((value >> (width - 1u - i)) & 1u) && (bit >> 3) < limit) dst[bit >> 3] |= (uint8_t)(0x80u >> (bit & 7u));
    }
}

/* The tokens of the stream in[0..n) from token start c0 up to the first token start >= e, from bit `at` of dst on; returns
 * the bits written, *exit_pos where the last token ends. */
static uint64_t tokens(uint8_t *dst, uint64_t limit, uint64_t at, const uint8_t *in, uint32_t n, uint32_t c0, uint32_t e, uint32_t *exit_pos)
{
    const uint64_t at0 = at;
    uint32_t c = c0;
    while (c < e) {
        unsigned off = 0;
        const unsigned len = lzs_oracle_search(in, n, c, &off);
        if (len < 2) { or_bits(dst, limit, at, in[c], 9); at += 9; c++; continue; }
        const unsigned first = len < 8 ? len : 8;
        if (off <= 127) { or_bits(dst, limit, at, (3u << 7) | off, 9); at += 9; } else { or_bits(dst, limit, at, (2u << 11) | off, 13); at += 13; }
        if (first <= 4) { or_bits(dst, limit, at, first - 2, 2); at += 2; } else { or_bits(dst, limit, at, 7 + first, 4); at += 4; }
        c += first;
        if (first == 8) {
            unsigned x;
            do {
                const unsigned lim = n - c < 15 ? n - c : 15;
                for (x = 0; x < lim && in[c + x] == in[c + x - off]; x++) {}
                or_bits(dst, limit, at, x, 4); at += 4;
                c += x;
            } while (x == 15);
        }
    }
    *exit_pos = c;
    return at - at0;
}

int lzs_hip_launch_compress_segments_batch(void *d_slots, size_t slot_stride, const void *d_in, const uint64_t *d_blk_at,
                                           const uint32_t *d_blk_len, const uint32_t *d_seg_block, const uint32_t *d_seg_start,
                                           uint32_t seg, uint32_t nseg, const uint32_t *d_entry, const uint8_t *d_dirty,
                                           uint32_t *d_exit, uint64_t *d_nbits, void *d_out, size_t out_stride, uint32_t out_cap,
                                           const uint64_t *d_bit_at, void *stream)
{
    (void)stream;
    g_bc_compress_launches++;
    if (d_out) g_bc_second_passes++;
    const uint64_t cap4 = ((uint64_t)out_cap + 3u) & ~(uint64_t)3u;
    for (uint32_t k = 0; k < nseg; k++) {
        if (d_dirty && !d_dirty[k]) continue;
        const uint32_t b = d_seg_block[k], s = d_seg_start[k], n = d_blk_len[b];
        const uint32_t e = n - s > seg ? s + seg : n, c0 = d_entry[k];
        if (c0 >= e) { d_exit[k] = c0; d_nbits[k] = 0; continue; }
        /* the block as a stream of its own: a copy of exactly its bytes */
        uint8_t *own = (uint8_t *)malloc(n);
        if (!own) return 2;
        memcpy(own, (const uint8_t *)d_in + d_blk_at[b], n);
        if (!d_out) {
            uint8_t *slot = (uint8_t *)d_slots + (size_t)k * slot_stride;
            memset(slot, 0, slot_stride);
            d_nbits[k] = tokens(slot, slot_stride, 0, own, n, c0, e, &d_exit[k]);
        } else {
            d_nbits[k] = tokens((uint8_t *)d_out + (size_t)b * out_stride, cap4, d_bit_at[k], own, n, c0, e, &d_exit[k]);
        }
        free(own);
    }
    return 0;
}

int lzs_hip_launch_stitch_segments_batch(void *d_out, size_t out_stride, uint32_t out_cap, const void *d_slots, size_t slot_stride,
                                         const uint64_t *d_bit_at, const uint64_t *d_nbits, const uint32_t *d_seg_block,
                                         const uint32_t *d_seg_start, const uint32_t *d_blk_len, uint32_t seg, uint32_t nseg, void *stream)
{
    (void)stream;
    g_bc_stitch_launches++;
    const uint64_t cap4 = ((uint64_t)out_cap + 3u) & ~(uint64_t)3u;
    for (uint32_t k = 0; k < nseg; k++) {
        const uint32_t b = d_seg_block[k];
        uint8_t *dst = (uint8_t *)d_out + (size_t)b * out_stride;
        const uint8_t *slot = (const uint8_t *)d_slots + (size_t)k * slot_stride;
        if (d_nbits[k] <= 8u * (uint64_t)slot_stride)            /* (else ORed in by the second pass) */
            for (uint64_t i = 0; i < d_nbits[k]; i++)
                if ((slot[i >> 3] >> (7u - (i & 7u))) & 1u) or_bits(dst, cap4, d_bit_at[k] + i, 1u, 1);
        if (d_blk_len[b] - d_seg_start[k] <= seg) or_bits(dst, cap4, d_bit_at[k] + d_nbits[k], 0x180u, 9);
    }
    return 0;
}

int lzs_hip_memset_rows(void *d, size_t pitch, int value, size_t width, size_t rows, void *stream)
{
    (void)stream;
    for (size_t r = 0; r < rows && width; r++) memset((uint8_t *)d + r * pitch, value, width);
    return 0;
}
