/*
 * oracle/lzs_oracle.c -- CPU restatement of the LZS one-shot codec, and plain models of one channel packet's decoding and
 * compression (lzs_oracle_decompress_channel, lzs_oracle_compress_channel: tests/test_channel_model.py,
 * tests/test_channel_encode_model.py hold them to the reference), and of what a segment border of the many-wavefront stream
 * decoders is (lzs_oracle_scan_segments: tests/test_stream_border_model.py) and of the segmented stream compressor
 * (lzs_oracle_compress_segments: tests/test_stream_compress_model.py).
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the shipped library (liblzs.so, the
 * lzs_compression_amd package) links, loads or calls this file.  Only tests/,
 * __graft_entry__.smoke() and the cpu_baseline leg of bench.py may use it, and
 * only as the checker, never as the thing measured as the product.
 *
 * Parity status: PINNED.  tests/test_oracle.py checks every function here
 * against (1) the reference's own golden vector and size laws
 * (c/src/test/test-lzs-decompression.c:34-96, c/src/test/test-lzs.c:44-167),
 * (2) fixtures minted from the compiled reference (tests/golden/), and, when
 * oracle/_ref/liblzs_ref.so is present, (3) the real reference live.
 *
 * This is a restatement of *behaviour*, written from the decision rule, not a
 * transcription: flat input indexing (no history ring), an exact 2-gram
 * previous-occurrence chain (no 12-bit hash, no uninitialised tables), a
 * 64-bit bit sink, and a bit-cursor decoder.  Reference lines each routine
 * answers to are cited at the routine.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* Wire-format constants: c/src/liblzs/lzs-common.h:38-53, lzs.h:57-60,
 * search cap c/src/liblzs/lzs-compression.c:62. */
enum {
    WINDOW      = 2047,   /* farthest offset a token can name (11 bits)        */
    SEARCH_CAP  = 12,     /* match length at which the search stops improving  */
    SHORT_MAX   = 127,    /* offsets <= this use the 7-bit form                */
    TOKEN_MAX   = 8,      /* longest length the first length code can carry    */
    NIBBLE_MAX  = 15      /* an extension nibble of 15 means "and continue"    */
};

/* ------------------------------------------------------------------ */
/* MSB-first bit sink with the reference's truncation rule:            */
/* bytes past the capacity are dropped, the count stops at capacity    */
/* (c/src/liblzs/lzs-compression.c:304-313, 456-465).                  */
/* ------------------------------------------------------------------ */
typedef struct {
    uint8_t *dst;
    size_t   cap;
    size_t   total;     /* bytes the untruncated stream would have had so far */
    uint64_t acc;       /* pending bits, right-aligned */
    unsigned pending;   /* how many */
} sink_t;

static void sink_put(sink_t *s, uint32_t value, unsigned width)
{
    s->acc = (s->acc << width) | value;
    s->pending += width;
    while (s->pending >= 8) {
        s->pending -= 8;
        if (s->total < s->cap)
            s->dst[s->total] = (uint8_t)(s->acc >> s->pending);
        s->total++;
    }
}

/* Number of equal leading bytes of in[a..] and in[b..], at most lim.
 * b < a; the two ranges may overlap (c/src/liblzs/lzs-compression.c:178-191). */
static unsigned common_prefix(const uint8_t *in, size_t a, size_t b, unsigned lim)
{
    unsigned k = 0;
    while (k < lim && in[a + k] == in[b + k])
        k++;
    return k;
}

/* Emit the (offset, first length code) of a match
 * (c/src/liblzs/lzs-compression.c:376-409, tables :100-124). */
static void put_match_head(sink_t *s, unsigned off, unsigned len_first)
{
    if (off <= SHORT_MAX)
        sink_put(s, (3u << 7) | off, 9);        /* 1 1 ooooooo        */
    else
        sink_put(s, (2u << 11) | off, 13);      /* 1 0 ooooooooooo    */
    if (len_first <= 4)
        sink_put(s, len_first - 2, 2);          /* 00 01 10           */
    else
        sink_put(s, 0xC + (len_first - 5), 4);  /* 1100 1101 1110 1111*/
}

/* ------------------------------------------------------------------ */
/* The search rule, brute force: the specification itself.             */
/* (c/src/liblzs/lzs-compression.c:322-363, equivalently               */
/*  c/src/liblzs/lzs-compression-simple.c:264-278) */
/* Returns the capped best length (0 or 1 = "no usable match") and the */
/* nearest offset that attains it.                                     */
/* ------------------------------------------------------------------ */
unsigned lzs_oracle_search(const uint8_t *in, size_t n, size_t c, unsigned *best_off)
{
    unsigned lim = (n - c < SEARCH_CAP) ? (unsigned)(n - c) : SEARCH_CAP;
    unsigned best = 0;
    size_t   reach = (c < WINDOW) ? c : WINDOW;
    *best_off = 0;
    if (lim < 2)
        return 0;
    for (size_t off = 1; off <= reach; off++) {
        unsigned l = common_prefix(in, c, c - off, lim);
        if (l > best) {
            best = l;
            *best_off = (unsigned)off;
            if (l == lim)
                break;
        }
    }
    return best;
}

/* Shared token loop.  `finder` selects brute force or the chained finder. */
typedef struct {
    int32_t *head;      /* 65536 entries: latest position of each exact 2-gram */
    int32_t *prev;      /* per position: previous position with the same 2-gram */
} chains_t;

static unsigned chained_search(const chains_t *ch, const uint8_t *in, size_t n, size_t c,
                               unsigned *best_off)
{
    unsigned lim = (n - c < SEARCH_CAP) ? (unsigned)(n - c) : SEARCH_CAP;
    unsigned best = 0;
    *best_off = 0;
    if (lim < 2)
        return 0;
    /* Every position whose first two bytes equal ours, nearest first.  Any
     * offset not on this list has common prefix <= 1 and can never win. */
    int32_t q = ch->head[((unsigned)in[c] << 8) | in[c + 1]];
    while (q >= 0 && c - (size_t)q <= WINDOW) {
        unsigned l = common_prefix(in, c, (size_t)q, lim);
        if (l > best) {
            best = l;
            *best_off = (unsigned)(c - (size_t)q);
            if (l == lim)
                break;
        }
        q = ch->prev[q];
    }
    return best;
}

/* What lzs_oracle_compress_channel counts (in order; oracle/__init__.py: CHANNEL_ENCODE_COUNTERS).  A token's source is
 * view[c - off, c - off + len); `start` is where the packet begins in the view. */
enum {
    CE_SRC_IN_HISTORY = 0,   /* matches whose source lies wholly before the packet                */
    CE_SRC_STRADDLES,        /* matches whose source starts before the packet and ends inside it  */
    CE_OFFSET_2047,          /* matches at the farthest offset                                    */
    CE_REACHES_VIEW_0,       /* matches whose source starts at byte 0 of the view                 */
    CE_SHORT_127,            /* the last offset of the 7-bit form                                 */
    CE_LONG_128,             /* the first offset of the 11-bit form                               */
    CE_NIBBLE_15,            /* extension nibbles of 15: the match continues                      */
    CE_EXT_ENDS_AT_END,      /* extended matches that end with the packet                         */
    CE_SEARCH_CUT_BY_END,    /* matches taken where fewer than 12 bytes were left to search       */
    CE_LAST_BYTE_LITERAL,    /* packets whose last byte is a literal                              */
    CE_FIRST_TOKEN_OFF_1,    /* packets whose first token is a match at offset 1                  */
    CE_CUT,                  /* packets cut at the capacity                                       */
    CE_COUNTERS
};

/* The token loop over in[0, n), the first token at `start`: what lies before it is only searched (`start` = 0: a whole
 * block).  The chains are built over in[0, start) too.  *total (may be NULL) receives the length of the uncut stream.
 * counters[] (may be NULL) are ADDED to; trace[] (may be NULL) receives up to max_tok records {position in the packet,
 * offset (0 = literal), bytes covered, bit position}, one a token, and *ntok the token count. */
static size_t compress_core(uint8_t *out, size_t cap, const uint8_t *in, size_t n, size_t start, int brute, size_t *total,
                            uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok)
{
    sink_t   s = { out, cap, 0, 0, 0 };
    chains_t ch = { NULL, NULL };
    size_t   c = start, inserted = 0, tok = 0;

    if (!brute) {
        ch.head = (int32_t *)malloc(65536 * sizeof(int32_t));
        ch.prev = (int32_t *)malloc((n ? n : 1) * sizeof(int32_t));
        if (!ch.head || !ch.prev) { free(ch.head); free(ch.prev); return (size_t)-1; }
        memset(ch.head, 0xFF, 65536 * sizeof(int32_t));
    }

    while (c < n) {
        unsigned off, len;
        size_t   at = c;
        uint64_t bit = (uint64_t)s.total * 8u + s.pending;
        int      extended = 0;
        if (!brute) {
            /* make every position before c searchable */
            for (; inserted < c; inserted++) {
                if (inserted + 1 < n) {
                    unsigned key = ((unsigned)in[inserted] << 8) | in[inserted + 1];
                    ch.prev[inserted] = ch.head[key];
                    ch.head[key] = (int32_t)inserted;
                }
            }
            len = chained_search(&ch, in, n, c, &off);
        } else {
            len = lzs_oracle_search(in, n, c, &off);
        }

        if (len < 2) {                                   /* :365-375 literal */
            sink_put(&s, in[c], 9);
            c += 1;
            off = 0;
            if (counters && c == n)
                counters[CE_LAST_BYTE_LITERAL]++;
        } else {
            unsigned first = len < TOKEN_MAX ? len : TOKEN_MAX;   /* :399 */
            if (counters && n - c < SEARCH_CAP)
                counters[CE_SEARCH_CUT_BY_END]++;
            put_match_head(&s, off, first);
            c += first;
            if (first == TOKEN_MAX) {                        /* :411-431 extension */
                unsigned e;
                extended = 1;
                do {
                    unsigned lim = (n - c < NIBBLE_MAX) ? (unsigned)(n - c) : NIBBLE_MAX;
                    e = common_prefix(in, c, c - off, lim);
                    sink_put(&s, e, 4);
                    c += e;
                    if (counters && e == NIBBLE_MAX)
                        counters[CE_NIBBLE_15]++;
                } while (e == NIBBLE_MAX);
            }
            if (counters) {
                size_t from = at - off, to = from + (c - at);            /* the source: in[from, to) */
                if (from < start && to <= start) counters[CE_SRC_IN_HISTORY]++;
                if (from < start && to > start)  counters[CE_SRC_STRADDLES]++;
                if (off == WINDOW)               counters[CE_OFFSET_2047]++;
                if (from == 0)                   counters[CE_REACHES_VIEW_0]++;
                if (off == SHORT_MAX)            counters[CE_SHORT_127]++;
                if (off == SHORT_MAX + 1)        counters[CE_LONG_128]++;
                if (extended && c == n)          counters[CE_EXT_ENDS_AT_END]++;
                if (at == start && off == 1)     counters[CE_FIRST_TOKEN_OFF_1]++;
            }
        }
        if (trace && tok < max_tok) {
            trace[4 * tok + 0] = (uint32_t)(at - start); trace[4 * tok + 1] = off;
            trace[4 * tok + 2] = (uint32_t)(c - at);     trace[4 * tok + 3] = (uint32_t)bit;
        }
        tok++;
    }
    /* End marker 1 1 0000000 then zero bits to the byte boundary (:449-466). */
    sink_put(&s, 0x180, 9);
    if (s.pending)
        sink_put(&s, 0, 8 - s.pending);

    free(ch.head);
    free(ch.prev);
    if (total)
        *total = s.total;
    if (ntok)
        *ntok = tok;
    if (counters && s.total > cap)
        counters[CE_CUT]++;
    return s.total < cap ? s.total : cap;
}

/* lzs_compress() semantics (c/src/liblzs/lzs-compression.c:249-467). */
size_t lzs_oracle_compress(uint8_t *out, size_t cap, const uint8_t *in, size_t n)
{
    return compress_core(out, cap, in, n, 0, 0, NULL, NULL, NULL, 0, NULL);
}

/* Same contract, brute-force finder: slow, but it *is* the written rule. */
size_t lzs_oracle_compress_brute(uint8_t *out, size_t cap, const uint8_t *in, size_t n)
{
    return compress_core(out, cap, in, n, 0, 1, NULL, NULL, NULL, 0, NULL);
}

/* ------------------------------------------------------------------ */
/* One packet of a channel, compressed (include/lzs/lzs_channels.h:    */
/* "Device-pointer channel compression"): what                         */
/* lzs_compress_incremental(add_end_marker) writes for in[0, n) on a   */
/* parameter block that has seen the channel's earlier packets.  The   */
/* rule is that of a block, on the view hist[0, h) | in[0, n), h <=    */
/* 2047, with the first token at h: offsets reach back min(position,   */
/* 2047) bytes of the view, lengths are capped by the end of the view, */
/* the nearest offset wins; the stream starts at bit 0 and ends with   */
/* the marker and its padding.                                         */
/*                                                                     */
/*  - out[] receives the stream cut at `cap`, as lzs_compress() cuts   */
/*    it; the return value is min(*total, cap), *total the uncut       */
/*    length.                                                          */
/*  - *status: END_MARKER | INPUT_FINISHED | INPUT_STARVED (0x07) if   */
/*    *total <= cap, else NO_OUTPUT_BUFFER_SPACE in the marker's place */
/*    (0x0B).                                                          */
/*  - new_hist[0, *new_h): the last min(2047, h + n) bytes of the view,*/
/*    cut or not.                                                      */
/*                                                                     */
/* `brute`: the written rule instead of the chained finder.  counters, */
/* trace, max_tok, ntok: as compress_core takes them.  Returns         */
/* (size_t)-1 if memory ran out.                                       */
/* ------------------------------------------------------------------ */
size_t lzs_oracle_compress_channel(uint8_t *out, size_t cap, const uint8_t *in, size_t n,
                                   const uint8_t *hist, size_t h, int brute, size_t *total,
                                   uint8_t *new_hist, size_t *new_h, uint8_t *status,
                                   uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok)
{
    size_t   view_n = h + n, uncut = 0;
    uint8_t *view = (uint8_t *)malloc(view_n + 1);
    if (!view)
        return (size_t)-1;
    if (h)
        memcpy(view, hist, h);
    if (n)
        memcpy(view + h, in, n);

    size_t got = compress_core(out, cap, view, view_n, h, brute, &uncut, counters, trace, max_tok, ntok);
    if (got != (size_t)-1) {
        size_t keep = view_n < WINDOW ? view_n : WINDOW;
        if (keep)
            memcpy(new_hist, view + view_n - keep, keep);
        *new_h = keep;
        *total = uncut;
        *status = uncut <= cap ? 0x07 : 0x0B;
    }
    free(view);
    return got;
}

/* ------------------------------------------------------------------ */
/* lzs_decompress() semantics (c/src/liblzs/lzs-decompression.c:156-412,*/
/* SURVEY.md App. A.4): stop at the first end marker, when the output  */
/* is full (also mid-copy), or when a field needs more bits than the   */
/* input still holds; sources before out[0] read as zero.              */
/* ------------------------------------------------------------------ */
typedef struct {
    const uint8_t *src;
    uint64_t       nbits;   /* total bits in the input */
    uint64_t       at;      /* cursor */
} cursor_t;

static uint64_t bits_left(const cursor_t *r) { return r->nbits - r->at; }

/* Next `w` (<= 16) bits, MSB first; bits past the end read as 0. */
static unsigned peek_bits(const cursor_t *r, unsigned w)
{
    unsigned v = 0;
    for (unsigned i = 0; i < w; i++) {
        uint64_t p = r->at + i;
        unsigned bit = (p < r->nbits) ? (r->src[p >> 3] >> (7 - (p & 7))) & 1u : 0u;
        v = (v << 1) | bit;
    }
    return v;
}

static unsigned take_bits(cursor_t *r, unsigned w)
{
    unsigned v = peek_bits(r, w);
    r->at += w;
    return v;
}

/* Copy `len` bytes from `off` back; 1 = output became full. (:346-365, :381-400) */
static int copy_back(uint8_t *out, size_t cap, size_t *count, unsigned off, unsigned len)
{
    for (unsigned i = 0; i < len; i++) {
        out[*count] = (*count >= off) ? out[*count - off] : 0;
        (*count)++;
        if (*count >= cap)
            return 1;
    }
    return 0;
}

size_t lzs_oracle_decompress(uint8_t *out, size_t cap, const uint8_t *in, size_t n)
{
    cursor_t r = { in, (uint64_t)n * 8u, 0 };
    size_t   count = 0;
    unsigned off = 0;
    int      extended = 0;

    for (;;) {
        if (bits_left(&r) == 0 || count >= cap)          /* :189, :200 */
            break;
        if (extended) {                                  /* :370-406 */
            if (bits_left(&r) < 4)
                break;
            unsigned e = take_bits(&r, 4);
            if (copy_back(out, cap, &count, off, e))
                break;
            if (e != NIBBLE_MAX)
                extended = 0;
            continue;
        }
        if (take_bits(&r, 1) == 0) {                     /* literal :217-233 */
            if (bits_left(&r) < 8)
                break;
            out[count++] = (uint8_t)take_bits(&r, 8);
            continue;
        }
        if (bits_left(&r) < 1)                           /* :238-241 */
            break;
        if (take_bits(&r, 1)) {                          /* short offset :248-260 */
            if (bits_left(&r) < 7)
                break;
            off = take_bits(&r, 7);
            if (off == 0)
                break;                                   /* end marker */
        } else {                                         /* long offset :272-279 */
            if (bits_left(&r) < 11)
                break;
            off = take_bits(&r, 11);
            if (off == 0)
                continue;                                /* :280 no copy, not an end marker */
        }
        /* length: 00 01 10 -> 2 3 4 ; 11xy -> 5 6 7 8 (:103-120, :325-342) */
        unsigned code = peek_bits(&r, 4);
        unsigned len, width;
        if (code < 0xC) { len = 2 + (code >> 2); width = 2; }
        else            { len = 5 + (code - 0xC); width = 4; }
        if (bits_left(&r) < width)
            break;
        r.at += width;
        if (len == TOKEN_MAX)
            extended = 1;
        if (copy_back(out, cap, &count, off, len))
            break;
    }
    return count;
}

/* ------------------------------------------------------------------ */
/* Token trace, for debugging kernels against the rule: writes up to   */
/* max_tok records {pos, off, len_total} (off 0 = literal) and returns */
/* the token count.  Not part of any reference interface.              */
/* ------------------------------------------------------------------ */
size_t lzs_oracle_trace(const uint8_t *in, size_t n, uint32_t *rec, size_t max_tok)
{
    size_t c = 0, t = 0;
    while (c < n) {
        unsigned off, len = lzs_oracle_search(in, n, c, &off);
        size_t start = c;
        if (len < 2) { off = 0; c += 1; }
        else {
            unsigned first = len < TOKEN_MAX ? len : TOKEN_MAX;
            c += first;
            if (first == TOKEN_MAX) {
                unsigned e;
                do {
                    unsigned lim = (n - c < NIBBLE_MAX) ? (unsigned)(n - c) : NIBBLE_MAX;
                    e = common_prefix(in, c, c - off, lim);
                    c += e;
                } while (e == NIBBLE_MAX);
            }
        }
        if (t < max_tok) {
            rec[3 * t + 0] = (uint32_t)start;
            rec[3 * t + 1] = off;
            rec[3 * t + 2] = (uint32_t)(c - start);
        }
        t++;
    }
    return t;
}

/* ------------------------------------------------------------------ */
/* One packet of a channel (include/lzs/lzs_channels.h: "Device-pointer */
/* channel decompression", and the status rule of lzs_batch.h), a bit   */
/* at a time.  The channel's history hist[0, h), h <= 2047, lies before */
/* the packet's output; what lies before the history reads as zero.     */
/*                                                                      */
/*  - The packet stops at its first end marker, at the end of its bits, */
/*    or at the capacity.  A token that lacks some of its bits, or that */
/*    finds no room at all, stops the packet and is not consumed.       */
/*  - The end marker needs no room.  It counts (END_MARKER) unless a    */
/*    copy was cut at the capacity before it; it also counts behind the */
/*    closing nibble 0 of a copy that exactly filled the output.        */
/*  - A long offset of 0 takes its 13 bits and copies nothing.          */
/*  - Status: END_MARKER (0x04) if the marker counted, else             */
/*    NO_OUTPUT_BUFFER_SPACE (0x08) if the output is full, else         */
/*    INPUT_STARVED | INPUT_FINISHED (0x03).                            */
/*  - The new history is the last min(2047, h + produced) bytes of      */
/*    history | output, whatever stopped the packet.                    */
/*                                                                      */
/* counters[] (may be NULL) are ADDED to, so that a test can prove its  */
/* inputs reached the edges.  trace[] (may be NULL) receives up to      */
/* max_tok records {output position, offset (0 = literal), bytes        */
/* produced, bit position}, one a token (a copy with all its nibbles    */
/* is one token), and *ntok the token count.  *stop_bit (may be NULL)   */
/* receives the bit at which the packet stopped: the marker's first bit */
/* if it stopped at one.                                                */
/* ------------------------------------------------------------------ */
enum {
    CH_ZERO_BYTES = 0,   /* bytes read as zero from before the history              */
    CH_CROSSING,         /* copies whose source runs from the history into the packet */
    CH_OVERLAP,          /* copies with offset < length                              */
    CH_LONG_SMALL,       /* offsets 1..127 written in the 11-bit form                */
    CH_LONG_ZERO,        /* long offset 0 tokens taken                               */
    CH_CUT,              /* copies cut at the capacity                               */
    CH_NIBBLE0_MARKER,   /* closing nibble 0 followed by a counted marker            */
    CH_NIBBLE0_FULL,     /* ... of which: the copy had exactly filled the output     */
    CH_COUNTERS
};

typedef struct {
    size_t   start;      /* output position of the open copy token's first byte */
    size_t   rec;        /* its record in the trace */
    unsigned off;
    int      open, from_history, from_packet;
} copy_t;

static void copy_close(copy_t *t, size_t count, uint64_t *ctr)
{
    if (!t->open)
        return;
    t->open = 0;
    if (!ctr)
        return;
    if (t->from_history && t->from_packet)
        ctr[CH_CROSSING]++;
    if (count - t->start > t->off)
        ctr[CH_OVERLAP]++;
}

size_t lzs_oracle_decompress_channel(uint8_t *out, size_t cap, const uint8_t *in, size_t n,
                                     const uint8_t *hist, size_t h,
                                     uint8_t *new_hist, size_t *new_h, uint8_t *status,
                                     uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok,
                                     uint64_t *stop_bit)
{
    cursor_t r = { in, (uint64_t)n * 8u, 0 };
    size_t   count = 0, tok = 0;
    int      extended = 0, cut = 0, marker = 0;
    copy_t   t = { 0, 0, 0, 0, 0, 0 };

    for (;;) {
        size_t   room = cap - count;
        size_t   at_start = count;
        uint64_t bit_start = r.at;
        unsigned len;

        if (extended) {
            /* a closing nibble 0 and the marker right behind it: the packet is whole even with no room left */
            if (!cut && bits_left(&r) >= 13 && peek_bits(&r, 13) == 0x180) {
                marker = 1;
                r.at += 4;
                if (counters) {
                    counters[CH_NIBBLE0_MARKER]++;
                    if (room == 0)
                        counters[CH_NIBBLE0_FULL]++;
                }
                break;
            }
            if (bits_left(&r) < 4 || room == 0)
                break;
            len = take_bits(&r, 4);
            if (len != NIBBLE_MAX)
                extended = 0;
        } else {
            copy_close(&t, count, counters);
            if (bits_left(&r) >= 1 && peek_bits(&r, 1) == 0) {          /* literal */
                if (bits_left(&r) < 9 || room == 0)
                    break;
                out[count++] = (uint8_t)take_bits(&r, 9);
                if (trace && tok < max_tok) {
                    trace[4 * tok + 0] = (uint32_t)at_start; trace[4 * tok + 1] = 0;
                    trace[4 * tok + 2] = 1;                  trace[4 * tok + 3] = (uint32_t)bit_start;
                }
                tok++;
                continue;
            }
            if (bits_left(&r) < 2)
                break;
            unsigned head, off;
            if (peek_bits(&r, 2) == 3) {                                 /* short offset */
                if (bits_left(&r) < 9)
                    break;
                off = peek_bits(&r, 9) & 0x7F;
                head = 9;
                if (off == 0) {                                          /* the end marker: needs no room */
                    marker = !cut;
                    break;
                }
            } else {                                                     /* long offset */
                if (bits_left(&r) < 13)
                    break;
                off = peek_bits(&r, 13) & 0x7FF;
                head = 13;
                if (off == 0) {                                          /* 13 bits, no copy */
                    if (room == 0)
                        break;
                    r.at += 13;
                    if (counters)
                        counters[CH_LONG_ZERO]++;
                    if (trace && tok < max_tok) {
                        trace[4 * tok + 0] = (uint32_t)at_start; trace[4 * tok + 1] = 0;
                        trace[4 * tok + 2] = 0;                  trace[4 * tok + 3] = (uint32_t)bit_start;
                    }
                    tok++;
                    continue;
                }
            }
            /* length: 00 01 10 -> 2 3 4 ; 11xy -> 5 6 7 8, then nibbles while they are 15 */
            unsigned width;
            if (bits_left(&r) < head + 2)
                break;
            r.at += head;
            unsigned code = peek_bits(&r, 4);
            if (code < 0xC) { len = 2 + (code >> 2); width = 2; }
            else            { len = 5 + (code - 0xC); width = 4; }
            if (bits_left(&r) < width || room == 0) {
                r.at = bit_start;
                break;
            }
            r.at += width;
            if (counters && head == 13 && off <= SHORT_MAX)
                counters[CH_LONG_SMALL]++;
            extended = (len == TOKEN_MAX);
            t.start = count; t.off = off; t.open = 1; t.from_history = t.from_packet = 0;
            t.rec = tok++;
            if (trace && t.rec < max_tok) {
                trace[4 * t.rec + 0] = (uint32_t)count; trace[4 * t.rec + 1] = off;
                trace[4 * t.rec + 2] = 0;               trace[4 * t.rec + 3] = (uint32_t)bit_start;
            }
        }

        /* the bytes of this code or nibble, as many as there is room for */
        for (unsigned i = 0; i < len; i++) {
            if (count == cap) {
                cut = 1;
                if (counters)
                    counters[CH_CUT]++;
                break;
            }
            uint8_t v = 0;
            if (count >= t.off) {
                v = out[count - t.off];
                t.from_packet = 1;
            } else {
                size_t back = t.off - count;                             /* 1 = the history's newest byte */
                t.from_history = 1;
                if (back <= h)
                    v = hist[h - back];
                else if (counters)
                    counters[CH_ZERO_BYTES]++;
            }
            out[count++] = v;
        }
        if (trace && t.rec < max_tok)
            trace[4 * t.rec + 2] = (uint32_t)(count - t.start);
    }
    copy_close(&t, count, counters);

    *status = marker ? 0x04 : (count >= cap ? 0x08 : 0x03);
    if (ntok)
        *ntok = tok;
    if (stop_bit)
        *stop_bit = r.at;

    /* the last min(2047, h + count) bytes of history | output, oldest first */
    size_t keep = h + count < WINDOW ? h + count : WINDOW;
    for (size_t i = 0; i < keep; i++) {
        size_t back = keep - i;                                          /* distance from the end of history | output */
        new_hist[i] = back <= count ? out[count - back] : hist[h - (back - count)];
    }
    *new_h = keep;
    return count;
}

/* ------------------------------------------------------------------ */
/* What a segment border IS, for the many-wavefront stream decoders     */
/* (DESIGN.md 3.6): the stream in[0, n) cut every `seg` bytes, walked   */
/* ONCE from bit 0, a bit at a time, under the one-shot rule            */
/* (lzs_oracle_decompress: the first end marker ends it) or, with       */
/* `file_rule`, the rule of lzs_decompress_concat (an end marker is     */
/* followed by zero bits to the next byte, and the walk goes on with    */
/* the history kept), up to `cap` bytes of output.  A token, and every  */
/* length nibble, is one STEP; a step belongs to the segment in which   */
/* its first bit lies, with all the bytes it produces.                  */
/*                                                                      */
/* rec[] receives SS_FIELDS words for each of the first max_seg         */
/* segments (the enum below); counters[] (may be NULL) are ADDED to     */
/* (the two *_MAX ones raised); trace[] (may be NULL) receives up to    */
/* max_tok records {bit, kind, offset, bytes produced, output position} */
/* of the steps the true walk took whole, *ntok their number.  Returns  */
/* the bytes produced (the sum of the segments'), (size_t)-1 if memory  */
/* ran out.                                                             */
/*                                                                      */
/* Second, for every segment k >= 1 the true walk reaches, the walk a   */
/* decoder takes that knows nothing: entered at the border's own bit in */
/* the normal state, a step at a time for as long as its steps start    */
/* inside the segment.  SS_MERGE: after how many steps it stands on a   */
/* step of the true walk in the same state (SS_NEVER: not inside the    */
/* segment); SS_PHANTOMS: the end markers it read before that (it goes  */
/* on behind them -- under the file rule from the next byte on).        */
/*                                                                      */
/* The model knows nothing of marks, rounds or origins: it says what    */
/* those arrive at.                                                     */
/* ------------------------------------------------------------------ */
enum {                      /* a segment's record */
    SS_ENTRY_BIT = 0,       /* bits past the border at which the first step that starts in the segment begins; SS_NEVER: the walk never got here */
    SS_ENTRY_EXT,           /* that step is a length nibble: an extension is running ...                                */
    SS_ENTRY_OFF,           /* ... at this offset                                                                        */
    SS_BYTES,               /* bytes the segment's steps produce                                                         */
    SS_OUT_START,           /* where they begin in the output                                                            */
    SS_STOP,                /* 0, or why the walk stopped at a step of this segment: 1 end marker, 2 the input ended (in a token or not), 3 the output was full */
    SS_MERGE,
    SS_PHANTOMS,
    SS_FIELDS
};
#define SS_NEVER 0xFFFFFFFFu

enum {                      /* step kinds: the trace, and the rows of the straddle matrix */
    SK_LIT = 0, SK_SHORT2, SK_LONG2, SK_SHORT4, SK_LONG4, SK_SHORT8, SK_LONG8,
    SK_FIRST_NIBBLE,        /* (matrix only: a nibble right behind its length-8 token, whatever its value -- counted under its value too) */
    SK_NIB15, SK_CLOSE0, SK_CLOSE1, SK_CLOSE14, SK_CLOSE_OTHER, SK_MARKER, SK_LONG_ZERO,
    SK_KINDS
};

enum {                      /* counters (oracle/__init__.py: SCAN_COUNTERS has the same layout) */
    SC_STRADDLE   = 0,                              /* [kind][b]: steps with b of their bits in front of a border, b = 0 .. width    */
    SC_B          = 24,
    SC_EXT_ENTRY  = SC_STRADDLE + SK_KINDS * SC_B,  /* [offset class][closing nibble, 15 = never closed]: segments entered in an extension */
    SC_CLOSE_AT   = SC_EXT_ENTRY + 8 * 16,          /* [d + 8]: closing nibbles that start d bits behind a border, d = -8 .. 7        */
    SC_ONES_SEG   = SC_CLOSE_AT + 16,               /* [next three bits set][entry bit & 3]: whole segments of 0xFF inside an extension */
    SC_ONES_RUN   = SC_ONES_SEG + 8,                /* [0 1 2 3 >=4]: extensions that cross a border, by the whole 0xFF segments they cover */
    SC_SHORT_ONES = SC_ONES_RUN + 5,                /* borders crossed by the extension of a short token 11 1111111 1111               */
    SC_PHANTOM    = SC_SHORT_ONES + 1,              /* [0 1 2 3 >=4]: segments by the end markers the guessed walk read before it merged */
    SC_NEVER      = SC_PHANTOM + 5,                 /* segments in which the guessed walk never merged                                  */
    SC_NEVER_RUN_MAX,                               /* ... the most of them in a row (raised, not added)                                */
    SC_SRC_OWN,                                     /* copying steps by where their source lies: the segment's own output,              */
    SC_SRC_OTHER,                                   /* another segment's,                                                              */
    SC_SRC_STRADDLE,                                /* both: it straddles the segment's output start;                                  */
    SC_SRC_BEFORE0,                                 /* (also) in front of out[0]                                                       */
    SC_BEFORE0_SEG,                                 /* [segment, 15 = later]: the last of these, by segment                             */
    SC_OFF_EDGE   = SC_BEFORE0_SEG + 16,            /* [1023 1024 1025 2046 2047]: match tokens at these offsets                        */
    SC_OFF_EDGE_FIRST = SC_OFF_EDGE + 5,            /* ... of which: producing the first byte of their segment's output                 */
    SC_CHAIN_MAX  = SC_OFF_EDGE_FIRST + 5,          /* the longest chain of copies of copies, in segments crossed (raised)              */
    SC_SMALL_SEGS,                                  /* segments the walk reaches that produce fewer than 2047 bytes                     */
    SC_COUNTERS
};

static unsigned offset_class(unsigned off, int short_form)
{
    return off == 1 ? 0 : off == 2 ? 1 : (off == 127 && short_form) ? 2 : off == 127 ? 3 : off == 128 ? 4
         : off == 1024 ? 5 : off == 2047 ? 6 : 7;
}

/* One step at r->at in the state (ext, off).  Returns 0 if the input lacks bits for it (nothing is consumed), else 1 with
 * *kind, *bytes (what it produces, uncut), the new state, and *form (1 = the match token was in the 7-bit form). */
static int scan_step(cursor_t *r, int *ext, unsigned *off, unsigned *kind, unsigned *bytes, int *form)
{
    *bytes = 0;
    if (*ext) {
        if (bits_left(r) < 4)
            return 0;
        unsigned e = take_bits(r, 4);
        *bytes = e;
        *kind = e == NIBBLE_MAX ? SK_NIB15 : e == 0 ? SK_CLOSE0 : e == 1 ? SK_CLOSE1 : e == 14 ? SK_CLOSE14 : SK_CLOSE_OTHER;
        if (e != NIBBLE_MAX)
            *ext = 0;
        return 1;
    }
    if (bits_left(r) < 1)
        return 0;
    if (peek_bits(r, 1) == 0) {
        if (bits_left(r) < 9)
            return 0;
        r->at += 9;
        *kind = SK_LIT; *bytes = 1;
        return 1;
    }
    if (bits_left(r) < 2)
        return 0;
    unsigned head, o;
    if (peek_bits(r, 2) == 3) {
        if (bits_left(r) < 9)
            return 0;
        o = peek_bits(r, 9) & 0x7F; head = 9; *form = 1;
        if (o == 0) { r->at += 9; *kind = SK_MARKER; return 1; }
    } else {
        if (bits_left(r) < 13)
            return 0;
        o = peek_bits(r, 13) & 0x7FF; head = 13; *form = 0;
        if (o == 0) { r->at += 13; *kind = SK_LONG_ZERO; return 1; }
    }
    if (bits_left(r) < head + 2)
        return 0;
    cursor_t q = *r;
    q.at += head;
    unsigned code = peek_bits(&q, 4), len, width;
    if (code < 0xC) { len = 2 + (code >> 2); width = 2; }
    else            { len = 5 + (code - 0xC); width = 4; }
    if (bits_left(&q) < width)
        return 0;
    r->at += head + width;
    *off = o; *bytes = len;
    *ext = len == TOKEN_MAX;
    *kind = len == TOKEN_MAX ? (head == 9 ? SK_SHORT8 : SK_LONG8) : width == 2 ? (head == 9 ? SK_SHORT2 : SK_LONG2)
                                                                                : (head == 9 ? SK_SHORT4 : SK_LONG4);
    return 1;
}

size_t lzs_oracle_scan_segments(const uint8_t *in, size_t n, size_t seg, int file_rule, size_t cap,
                                uint32_t *rec, size_t max_seg, uint64_t *counters,
                                uint32_t *trace, size_t max_tok, size_t *ntok)
{
    static const unsigned edges[5] = { 1023, 1024, 1025, 2046, 2047 };
    const uint64_t nbits = (uint64_t)n * 8u, segbits = (uint64_t)seg * 8u;
    const size_t   nseg = seg ? (n + seg - 1) / seg : 0;
    const size_t   room = cap < 30 * n + 16 ? cap : 30 * n + 16;          /* a nibble gives at most 15 bytes */
    uint32_t *state_at = (uint32_t *)calloc((size_t)nbits + 1, sizeof(uint32_t));   /* per bit: 0, or 1 | ext << 1 | offset << 2 of the true step there */
    uint16_t *hops = (uint16_t *)malloc((room + 1) * sizeof(uint16_t));   /* per output byte: segments its chain of copies crosses */
    uint64_t  zero[SC_COUNTERS];
    uint64_t *ctr = counters ? counters : zero;
    if (!state_at || !hops || seg == 0) { free(state_at); free(hops); return (size_t)-1; }
    memset(zero, 0, sizeof(zero));
    for (size_t k = 0; k < nseg && k < max_seg; k++) {
        uint32_t *s = rec + k * SS_FIELDS;
        s[SS_ENTRY_BIT] = SS_NEVER; s[SS_ENTRY_EXT] = s[SS_ENTRY_OFF] = s[SS_BYTES] = s[SS_OUT_START] = s[SS_STOP] = 0;
        s[SS_MERGE] = SS_NEVER; s[SS_PHANTOMS] = 0;
    }

    /* ---- the true walk */
    cursor_t r = { in, nbits, 0 };
    size_t   count = 0, tok = 0, reached = 0;       /* reached: segments entered so far */
    unsigned off = 0, prev_kind = SK_KINDS;
    int      ext = 0, form = 0, stop = 0;
    unsigned ext_ones = 0, ext_crossed = 0;         /* the extension running: whole 0xFF segments it covered, borders it crossed */
    size_t   seg_out_start = 0;
    unsigned chain_max = 0;

    while (!stop) {
        if (count >= cap)       { stop = 3; break; }      /* (also where the input ends with the step that filled it) */
        if (bits_left(&r) == 0) { stop = 2; break; }
        const uint64_t at = r.at;
        const size_t   k = (size_t)(at / segbits);
        if (k >= reached) {                         /* the first step that starts in segment k */
            reached = k + 1;
            seg_out_start = count;
            if (k < max_seg) {
                uint32_t *s = rec + k * SS_FIELDS;
                s[SS_ENTRY_BIT] = (uint32_t)(at - k * segbits); s[SS_ENTRY_EXT] = (uint32_t)ext; s[SS_ENTRY_OFF] = ext ? off : 0;
                s[SS_OUT_START] = (uint32_t)count;
            }
            if (ext && k > 0) {
                ext_crossed++;
                if (off == SHORT_MAX && form) ctr[SC_SHORT_ONES]++;
                /* a whole segment of 0xFF inside the extension */
                if ((k + 1) * seg <= n) {
                    size_t i = 0;
                    while (i < seg && in[k * seg + i] == 0xFF) i++;
                    if (i == seg) {
                        const int next3 = (k + 1) * seg < n && (in[(k + 1) * seg] & 0xE0) == 0xE0;
                        ctr[SC_ONES_SEG + 4 * next3 + ((at - k * segbits) & 3)]++;
                        ext_ones++;
                    }
                }
            }
        }
        const int      was_ext = ext, was_form = form;
        const unsigned was_off = off;
        unsigned kind = 0, bytes = 0;
        if (!scan_step(&r, &ext, &off, &kind, &bytes, &form)) {
            /* the input ends inside this step; the one-shot decoder still takes the type bits it has (no bytes come of them) */
            stop = 2;
            break;
        }
        state_at[at] = 1u | ((uint32_t)was_ext << 1) | ((was_ext ? was_off : 0u) << 2);
        const unsigned width = (unsigned)(r.at - at);
        /* borders this step touches: b bits of it in front (a step is shorter than a segment: one border at most, or one at each end) */
        for (uint64_t B = (at + segbits - 1) / segbits * segbits; B <= at + width && B < nbits; B += segbits) {
            if (B == 0) continue;
            const unsigned b = (unsigned)(B - at);
            ctr[SC_STRADDLE + kind * SC_B + b]++;
            if (was_ext && (prev_kind == SK_SHORT8 || prev_kind == SK_LONG8))
                ctr[SC_STRADDLE + SK_FIRST_NIBBLE * SC_B + b]++;
        }
        if (was_ext && kind != SK_NIB15) {
            /* a closing nibble: d bits behind the nearest border */
            const uint64_t lo = at / segbits * segbits, hi = lo + segbits;
            if (at - lo < 8 && lo > 0) ctr[SC_CLOSE_AT + 8 + (unsigned)(at - lo)]++;
            if (hi - at <= 8 && hi < nbits) ctr[SC_CLOSE_AT + 8 - (unsigned)(hi - at)]++;
            if (ext_crossed) {                      /* every segment it entered, by the nibble that closes it now */
                ctr[SC_EXT_ENTRY + 16 * offset_class(was_off, was_form) + bytes] += ext_crossed;
                ctr[SC_ONES_RUN + (ext_ones < 4 ? ext_ones : 4)]++;
            }
            ext_crossed = 0; ext_ones = 0;
        }
        if (kind == SK_MARKER) {
            if (trace && tok < max_tok) {
                trace[5 * tok + 0] = (uint32_t)at; trace[5 * tok + 1] = kind; trace[5 * tok + 2] = 0; trace[5 * tok + 3] = 0; trace[5 * tok + 4] = (uint32_t)count;
            }
            tok++;
            prev_kind = kind;
            if (!file_rule) { stop = 1; if (k < max_seg) rec[k * SS_FIELDS + SS_STOP] = 1; break; }
            r.at = (r.at + 7u) & ~(uint64_t)7u;
            if (r.at > nbits) r.at = nbits;
            continue;
        }
        /* the bytes of this step, as many as there is room for */
        const size_t at_out = count;
        if (bytes && kind != SK_LIT) {
            int own = 0, other = 0, before0 = 0;
            for (unsigned i = 0; i < bytes && count < cap; i++, count++) {
                unsigned h = 0;
                if (count < off) before0 = 1;
                else {
                    const size_t s = count - off;
                    if (s >= seg_out_start) { own = 1; h = hops[s]; }
                    else                    { other = 1; h = hops[s] + 1u; }
                }
                hops[count] = (uint16_t)(h < 0xFFFF ? h : 0xFFFF);
                if (h > chain_max) chain_max = h;
            }
            if (own && other)  ctr[SC_SRC_STRADDLE]++;
            else if (own)      ctr[SC_SRC_OWN]++;
            else if (other)    ctr[SC_SRC_OTHER]++;
            if (before0) { ctr[SC_SRC_BEFORE0]++; ctr[SC_BEFORE0_SEG + (k < 15 ? k : 15)]++; }
            if (!was_ext)
                for (int e = 0; e < 5; e++)
                    if (off == edges[e]) { ctr[SC_OFF_EDGE + e]++; if (at_out == seg_out_start) ctr[SC_OFF_EDGE_FIRST + e]++; }
        } else if (bytes) {
            hops[count++] = 0;
        }
        if (k < max_seg) rec[k * SS_FIELDS + SS_BYTES] += (uint32_t)(count - at_out);
        if (trace && tok < max_tok) {
            trace[5 * tok + 0] = (uint32_t)at; trace[5 * tok + 1] = kind; trace[5 * tok + 2] = (kind == SK_LIT || kind == SK_LONG_ZERO) ? 0 : off;
            trace[5 * tok + 3] = (uint32_t)(count - at_out); trace[5 * tok + 4] = (uint32_t)at_out;
        }
        tok++;
        prev_kind = kind;
    }
    if (stop != 1 && nseg) {
        const uint64_t last = r.at < nbits ? r.at : nbits - 1;
        const size_t   k = (size_t)(last / segbits);
        if (k < max_seg) rec[k * SS_FIELDS + SS_STOP] = (uint32_t)stop;
    }
    if (ext_crossed)                                /* an extension still open when the walk stopped: never closed */
        ctr[SC_EXT_ENTRY + 16 * offset_class(off, form) + 15] += ext_crossed;
    if (ntok) *ntok = tok;
    if (chain_max > ctr[SC_CHAIN_MAX]) ctr[SC_CHAIN_MAX] = chain_max;

    /* ---- the guessed walk of every segment the true walk reached */
    uint64_t never_run = 0;
    for (size_t k = 0; k < reached; k++) {
        uint32_t *s = k < max_seg ? rec + k * SS_FIELDS : NULL;
        if (s && s[SS_BYTES] < WINDOW) ctr[SC_SMALL_SEGS]++;
        if (k == 0) { if (s) s[SS_MERGE] = 0; continue; }
        cursor_t g = { in, nbits, (uint64_t)k * segbits };
        const uint64_t end = g.at + segbits;
        unsigned g_off = 0, g_kind = 0, g_bytes = 0, steps = 0, phantoms = 0;
        int      g_ext = 0, g_form = 0, merged = 0;
        while (g.at < end && g.at < nbits) {
            if (state_at[g.at] == (1u | ((uint32_t)g_ext << 1) | ((g_ext ? g_off : 0u) << 2))) { merged = 1; break; }
            if (!scan_step(&g, &g_ext, &g_off, &g_kind, &g_bytes, &g_form))
                break;
            steps++;
            if (g_kind == SK_MARKER) {
                phantoms++;
                if (file_rule) g.at = (g.at + 7u) & ~(uint64_t)7u;
            }
        }
        if (s) { s[SS_MERGE] = merged ? steps : SS_NEVER; s[SS_PHANTOMS] = phantoms; }
        ctr[SC_PHANTOM + (phantoms < 4 ? phantoms : 4)]++;
        if (!merged) {
            ctr[SC_NEVER]++;
            if (++never_run > ctr[SC_NEVER_RUN_MAX]) ctr[SC_NEVER_RUN_MAX] = never_run;
        } else
            never_run = 0;
    }
    free(state_at); free(hops);
    return count;
}

/* ------------------------------------------------------------------ */
/* What a segment border IS, for the segmented stream compressor        */
/* (DESIGN.md 3.5): in[0, n) cut every `seg` bytes (a multiple of 64,   */
/* >= 256), parsed ONCE from byte 0 by the token loop of compress_core  */
/* (the chained finder, or with `brute` the written rule).  A token,    */
/* with all its length nibbles, belongs to the segment in which it      */
/* STARTS.  The model knows nothing of slots, rounds, chains or warm-up */
/* windows: it says what they arrive at.                                */
/*                                                                      */
/* rec[] receives CP_FIELDS 64-bit words for each of the first max_seg  */
/* segments (the enum below).  Second, for every segment k >= 1, the    */
/* walk a workgroup takes that knows nothing: tokens from k * seg       */
/* itself for as long as they start inside the segment (CP_GUESS_MERGE: */
/* after how many tokens it stands on a token start of the true walk,   */
/* CP_NEVER: not inside the segment; CP_GUESS_EXIT: where it ends).     */
/* Third, the host's rounds exactly as stream_compress_piece() writes   */
/* them (csrc/lzs_stream.c), on the model's own walks: everyone enters  */
/* at max(k * seg, c_first) -- c_first = 0 here --, a segment entered   */
/* at or behind its end leaves where it was entered, and a segment is   */
/* redone when its predecessor's exit differs from its entry.           */
/* rounds[r] (up to max_rounds) receives the segments to redo after     */
/* round r, *nrounds the number of rounds; the rule is deterministic,   */
/* the device must give these numbers.                                  */
/*                                                                      */
/* counters[] (may be NULL) are ADDED to (the *_MAX ones raised), so    */
/* that a test can prove its inputs reached the edges; trace[] (may be  */
/* NULL) receives up to max_tok records {position, offset (0 =          */
/* literal), bytes covered, bit position} of the true walk, *ntok       */
/* their number.  Returns the bits of all tokens (the end marker and    */
/* its padding not counted), (size_t)-1 if memory ran out or seg is not */
/* a segment size.                                                      */
/* ------------------------------------------------------------------ */
enum {                      /* a segment's record */
    CP_ENTRY = 0,           /* where its first token starts; CP_NEVER: a match ran over all of it                 */
    CP_EXIT,                /* where its last token ends (an empty segment: where it was run over to)             */
    CP_TOKENS,
    CP_BITS,
    CP_BIT_AT,              /* the prefix sum of the bits before it                                               */
    CP_EMPTY,
    CP_OVERSIZED,           /* the host's rule: bits > 8 * align16(LZS_COMPRESSED_MAX(seg))                       */
    CP_GUESS_MERGE,
    CP_GUESS_EXIT,
    CP_REDONE,              /* rounds after round 0 in which the host's rule ran it again                         */
    CP_ROUND_EXIT,          /* the exit the rounds arrived at (the test: == CP_EXIT)                              */
    CP_FIELDS
};
#define CP_NEVER 0xFFFFFFFFFFFFFFFFull

enum {                      /* rows of CC_LAST: the last token of a segment that has a border behind it */
    CK_LIT = 0, CK_SHORT27, CK_LONG27, CK_EXT0, CK_EXT1, CK_EXT2, CK_EXT3_39, CK_EXT40,   /* length 8 and more: by its nibbles of 15 */
    CK_KINDS
};
enum { CC_PAST = 21 };      /* columns of CC_LAST: ends 0 .. 16 bytes past the border; 17: farther, inside the next segment; 18 19 20: past 1, 2, >= 3 whole segments */

enum {                      /* counters (oracle/__init__.py: CompressCounters has the same layout) */
    CC_LAST       = 0,                              /* [kind][past]                                                                  */
    CC_LAST_CLOSE = CC_LAST + CK_KINDS * CC_PAST,   /* [0 1 14 other]: closing nibbles of last tokens that end past their border     */
    CC_LAST_START = CC_LAST_CLOSE + 4,              /* [s]: last tokens that are matches and start s = 1 .. 8 bytes before the border (0: farther) */
    CC_ONE_TOKEN_LAST_BYTE = CC_LAST_START + 9,     /* segments entered at their last byte: one token                                */
    CC_ENTRY_MOD64,                                 /* [c0 & 63]: entries of non-empty segments k >= 1                               */
    CC_FIRST_OFF  = CC_ENTRY_MOD64 + 64,            /* [2047 2046 2040 1][warm-up window (c0 & ~63) - 2176 clamped: at 0, the first segment beyond, later ones]: first tokens of segments k >= 1 that are matches at these offsets */
    CC_FIRST_STRADDLE = CC_FIRST_OFF + 12,          /* ... of any offset, whose source has a segment border inside it                */
    CC_FIRST_FAR_LEN,                               /* [2 3]: first tokens at offset 2047 of exactly this length, warm-up not at 0   */
    CC_MERGE      = CC_FIRST_FAR_LEN + 2,           /* [0 1 2 3-4 >=5 never]: guessed walks by the tokens before they fall in step   */
    CC_ONE_ROUND  = CC_MERGE + 6,                   /* inputs of two segments and more settled by round 0                            */
    CC_ROUNDS_MAX,                                  /* the most rounds (raised)                                                      */
    CC_FIX_CHANGES_EXIT,                            /* segments whose true entry is not their border: the exit differs from the guessed walk's, */
    CC_FIX_KEEPS_EXIT,                              /* ... or does not                                                              */
    CC_NEVER_RUN_MAX,                               /* the most non-empty segments in a row whose guessed walks never merge (raised) */
    CC_LONG_MATCH,                                  /* [offset 1, 2, 300]: the most segments one token starts in or runs over (raised) */
    CC_BIT_AT_MOD32 = CC_LONG_MATCH + 3,            /* [bit_at % 32] of non-empty segments                                           */
    CC_NBITS_MOD32 = CC_BIT_AT_MOD32 + 32,          /* [bits % 32] of non-empty segments                                             */
    CC_UNDER_32   = CC_NBITS_MOD32 + 32,            /* non-empty segments of fewer than 32 bits                                      */
    CC_WORD_SHARE_MAX,                              /* the most non-empty segments with bits in one 32-bit word of the stream (raised) */
    CC_EMPTY_BETWEEN_SHARERS,                       /* runs of empty segments between two that put bits into one word                */
    CC_TOTAL_MOD32,                                 /* [total % 32]: where the end marker starts                                     */
    CC_MARKER_BEHIND_EMPTY = CC_TOTAL_MOD32 + 32,   /* inputs whose last segment is empty                                            */
    CC_MARKER_BEHIND_OVERSIZED,                     /* inputs whose last non-empty segment is oversized (the last segment itself cannot be: its tokens end with the input) */
    CC_MARGIN,                                      /* [d + 8]: segments whose bits are the slot's + d, d = -8 .. 8; [17]: more than 4096 over */
    CC_OVER_BIT_AT = CC_MARGIN + 18,                /* [0, 1-31, 32-2016, >= 2017]: oversized segments by bit_at % 2048              */
    CC_OVER_SEG0  = CC_OVER_BIT_AT + 4,             /* segment 0 oversized                                                           */
    CC_OVER_TWO,                                    /* inputs with two oversized segments and more                                   */
    CC_OVER_EMPTIES_ONE_TOKEN,                      /* an oversized segment, empty ones, then a one-token segment                    */
    CC_LEN_MOD,                                     /* [n % seg: 1 63 64 255 0]                                                      */
    CC_END_CLOSE  = CC_LEN_MOD + 5,                 /* [0 14]: the last token is a match of 8 and more that reaches n with this closing nibble */
    CC_END_ONE_SHORT = CC_END_CLOSE + 2,            /* a match that ends one byte before n, then a literal                           */
    CC_COUNTERS
};

typedef struct { uint32_t end, bits, nib15; uint16_t off; uint8_t close; } cp_tok_t;

/* the token that starts at c: compress_core's decision, as a function of (input, position) */
static void cp_token(const uint8_t *in, size_t n, size_t c, int brute, const int32_t *prev, cp_tok_t *t)
{
    unsigned off = 0, best = 0;
    unsigned lim = (n - c < SEARCH_CAP) ? (unsigned)(n - c) : SEARCH_CAP;
    if (brute)
        best = lzs_oracle_search(in, n, c, &off);
    else if (lim >= 2) {
        /* every earlier position with our 2-gram, nearest first: chained_search on chains that hold all of in[0, c) */
        for (int32_t q = prev[c]; q >= 0 && c - (size_t)q <= WINDOW; q = prev[q]) {
            unsigned l = common_prefix(in, c, (size_t)q, lim);
            if (l > best) {
                best = l; off = (unsigned)(c - (size_t)q);
                if (l == lim) break;
            }
        }
    }
    t->nib15 = 0; t->close = 0xFF;
    if (best < 2) { t->end = (uint32_t)c + 1; t->bits = 9; t->off = 0; return; }
    unsigned first = best < TOKEN_MAX ? best : TOKEN_MAX;
    size_t   e = c + first;
    t->off = (uint16_t)off;
    t->bits = (off <= SHORT_MAX ? 9u : 13u) + (first <= 4 ? 2u : 4u);
    if (first == TOKEN_MAX) {
        unsigned x;
        do {
            unsigned l = (n - e < NIBBLE_MAX) ? (unsigned)(n - e) : NIBBLE_MAX;
            x = common_prefix(in, e, e - off, l);
            e += x; t->bits += 4;
            if (x == NIBBLE_MAX) t->nib15++;
        } while (x == NIBBLE_MAX);
        t->close = (uint8_t)x;
    }
    t->end = (uint32_t)e;
}

size_t lzs_oracle_compress_segments(const uint8_t *in, size_t n, size_t seg, int brute,
                                    uint64_t *rec, size_t max_seg, uint32_t *rounds, size_t max_rounds, size_t *nrounds,
                                    uint64_t *counters, uint32_t *trace, size_t max_tok, size_t *ntok)
{
    static const unsigned first_offs[4] = { 2047, 2046, 2040, 1 }, long_offs[3] = { 1, 2, 300 };
    if (seg < 256 || (seg & 63) || n >= 0x7FFFFFFFu)
        return (size_t)-1;
    const size_t   nseg = n ? (n + seg - 1) / seg : 1;
    const uint64_t slot_bits = 8u * (uint64_t)(((seg + (seg + 7) / 8 + 3) + 15u) & ~(size_t)15u);
    uint64_t  zero[CC_COUNTERS];
    uint64_t *ctr = counters ? counters : zero;
    cp_tok_t *memo = (cp_tok_t *)calloc(n + 1, sizeof(cp_tok_t));        /* end == 0: not asked for yet */
    uint8_t  *is_start = (uint8_t *)calloc(n + 1, 1);
    int32_t  *prev = (int32_t *)malloc((n + 1) * sizeof(int32_t)), *head = (int32_t *)malloc(65536 * sizeof(int32_t));
    uint64_t *s = (uint64_t *)calloc(nseg * CP_FIELDS, sizeof(uint64_t));  /* all records, whatever max_seg is */
    uint32_t *entry = (uint32_t *)malloc(nseg * sizeof(uint32_t)), *exitp = (uint32_t *)malloc(nseg * sizeof(uint32_t));
    uint8_t  *dirty = (uint8_t *)malloc(nseg);
    size_t    result = (size_t)-1;
    if (!memo || !is_start || !prev || !head || !s || !entry || !exitp || !dirty)
        goto done;
    memset(zero, 0, sizeof(zero));
    memset(head, 0xFF, 65536 * sizeof(int32_t));
    for (size_t i = 0; i < n; i++) {
        prev[i] = -1;
        if (i + 1 < n) {
            unsigned key = ((unsigned)in[i] << 8) | in[i + 1];
            prev[i] = head[key]; head[key] = (int32_t)i;
        }
    }
#define TOKEN(c) (memo[c].end ? &memo[c] : (cp_token(in, n, (c), brute, prev, &memo[c]), &memo[c]))
#define SEG_END(k) (((k) + 1) * seg < n ? ((k) + 1) * seg : n)

    /* ---- the one walk */
    for (size_t k = 0; k < nseg; k++) { s[k * CP_FIELDS + CP_ENTRY] = CP_NEVER; s[k * CP_FIELDS + CP_EMPTY] = 1; }
    size_t   tok = 0;
    uint64_t bit = 0;
    for (size_t c = 0; c < n; ) {
        const cp_tok_t *t = TOKEN(c);
        const size_t k = c / seg;
        uint64_t *r = s + k * CP_FIELDS;
        is_start[c] = 1;
        if (r[CP_EMPTY]) { r[CP_EMPTY] = 0; r[CP_ENTRY] = c; }
        r[CP_EXIT] = t->end; r[CP_TOKENS]++; r[CP_BITS] += t->bits;
        if (trace && tok < max_tok) {
            trace[4 * tok + 0] = (uint32_t)c; trace[4 * tok + 1] = t->off; trace[4 * tok + 2] = t->end - (uint32_t)c; trace[4 * tok + 3] = (uint32_t)bit;
        }
        tok++; bit += t->bits;
        /* the segments this token starts in or runs over */
        for (int o = 0; o < 3; o++)
            if (t->off == long_offs[o]) {
                const uint64_t over = (t->end - 1) / seg - k + 1;
                if (over > ctr[CC_LONG_MATCH + o]) ctr[CC_LONG_MATCH + o] = over;
            }
        c = t->end;
    }
    if (ntok) *ntok = tok;
    result = (size_t)bit;
    {
        uint64_t at = 0, exit_before = 0;
        for (size_t k = 0; k < nseg; k++) {
            uint64_t *r = s + k * CP_FIELDS;
            if (r[CP_EMPTY]) r[CP_EXIT] = exit_before;
            exit_before = r[CP_EXIT];
            r[CP_BIT_AT] = at; at += r[CP_BITS];
            r[CP_OVERSIZED] = r[CP_BITS] > slot_bits;
        }
    }

    /* ---- the guessed walk of every segment behind the first */
    s[CP_GUESS_MERGE] = 0; s[CP_GUESS_EXIT] = s[CP_EXIT];
    uint64_t never_run = 0;
    for (size_t k = 1; k < nseg; k++) {
        uint64_t *r = s + k * CP_FIELDS;
        const size_t e = SEG_END(k);
        size_t   g = k * seg;
        uint64_t steps = 0, merged = CP_NEVER;
        while (g < e) {
            if (is_start[g]) { merged = steps; break; }
            g = TOKEN(g)->end; steps++;
        }
        r[CP_GUESS_MERGE] = merged;
        r[CP_GUESS_EXIT] = merged == CP_NEVER ? g : r[CP_EXIT];
        ctr[CC_MERGE + (merged == CP_NEVER ? 5 : merged >= 5 ? 4 : merged >= 3 ? 3 : merged)]++;
        if (merged == CP_NEVER && !r[CP_EMPTY]) { if (++never_run > ctr[CC_NEVER_RUN_MAX]) ctr[CC_NEVER_RUN_MAX] = never_run; }
        else never_run = 0;
        if (!r[CP_EMPTY] && r[CP_ENTRY] != k * seg)
            ctr[r[CP_GUESS_EXIT] != r[CP_EXIT] ? CC_FIX_CHANGES_EXIT : CC_FIX_KEEPS_EXIT]++;
    }

    /* ---- the host's rounds (stream_compress_piece: the loop over `round`), c_first = 0 */
    size_t nr = 0;
    for (size_t k = 0; k < nseg; k++) { entry[k] = (uint32_t)(k * seg); dirty[k] = 1; exitp[k] = entry[k]; }
    for (size_t ndirty = nseg; ndirty; nr++) {
        for (size_t k = 0; k < nseg; k++) {
            if (!dirty[k]) continue;
            const size_t e = SEG_END(k);
            size_t c = entry[k];
            while (c < e) c = TOKEN(c)->end;          /* (entered at or behind its end: it leaves where it was entered) */
            exitp[k] = (uint32_t)c;
            if (nr) s[k * CP_FIELDS + CP_REDONE]++;
        }
        ndirty = 0; dirty[0] = 0;
        for (size_t k = 1; k < nseg; k++) {
            dirty[k] = exitp[k - 1] != entry[k];
            if (dirty[k]) { entry[k] = exitp[k - 1]; ndirty++; }
        }
        if (rounds && nr < max_rounds) rounds[nr] = (uint32_t)ndirty;
    }
    if (nrounds) *nrounds = nr;
    for (size_t k = 0; k < nseg; k++) s[k * CP_FIELDS + CP_ROUND_EXIT] = exitp[k];
    if (nseg >= 2 && nr == 1) ctr[CC_ONE_ROUND]++;
    if (nr > ctr[CC_ROUNDS_MAX]) ctr[CC_ROUNDS_MAX] = nr;

    /* ---- what the records reach */
    {
        size_t   noversized = 0, last_full = nseg;          /* last_full: the non-empty segment before the one looked at */
        uint64_t word = CP_NEVER, sharers = 0;
        for (size_t k = 0; k < nseg; k++) {
            const uint64_t *r = s + k * CP_FIELDS;
            const int64_t  margin = (int64_t)r[CP_BITS] - (int64_t)slot_bits;
            if (margin >= -8 && margin <= 8) ctr[CC_MARGIN + (margin + 8)]++;
            if (margin > 4096) ctr[CC_MARGIN + 17]++;
            if (r[CP_EMPTY]) continue;
            const size_t border = (k + 1) * seg, c0 = (size_t)r[CP_ENTRY];
            size_t       last = c0;                         /* the segment's last token */
            while (TOKEN(last)->end < r[CP_EXIT]) last = TOKEN(last)->end;
            const cp_tok_t *t = TOKEN(last), *f = TOKEN(c0);
            size_t empties = 0;
            while (k + 1 + empties < nseg && s[(k + 1 + empties) * CP_FIELDS + CP_EMPTY]) empties++;
            if (border < n) {
                const unsigned kind = !t->off ? CK_LIT : t->close == 0xFF ? (t->off <= SHORT_MAX ? CK_SHORT27 : CK_LONG27)
                                    : t->nib15 == 0 ? CK_EXT0 : t->nib15 == 1 ? CK_EXT1 : t->nib15 == 2 ? CK_EXT2 : t->nib15 < 40 ? CK_EXT3_39 : CK_EXT40;
                const size_t d = t->end - border;
                const unsigned past = empties >= 3 ? 20 : empties == 2 ? 19 : empties == 1 ? 18 : d > 16 ? 17 : (unsigned)d;
                ctr[CC_LAST + kind * CC_PAST + past]++;
                if (t->close != 0xFF && d > 0) ctr[CC_LAST_CLOSE + (t->close == 0 ? 0 : t->close == 1 ? 1 : t->close == 14 ? 2 : 3)]++;
                if (t->off) ctr[CC_LAST_START + (border - last <= 8 ? border - last : 0)]++;
            }
            if (c0 == SEG_END(k) - 1 && border <= n) ctr[CC_ONE_TOKEN_LAST_BYTE]++;
            if (k >= 1) {
                ctr[CC_ENTRY_MOD64 + (c0 & 63)]++;
                if (f->off) {
                    const size_t c64 = c0 & ~(size_t)63;
                    const unsigned warm = c64 <= 2176 ? 0 : k <= 2176 / seg + 1 ? 1 : 2;
                    const size_t from = c0 - f->off, to = from + (f->end - c0);
                    for (int o = 0; o < 4; o++)
                        if (f->off == first_offs[o]) ctr[CC_FIRST_OFF + 3 * o + warm]++;
                    if ((to - 1) / seg != from / seg) ctr[CC_FIRST_STRADDLE]++;
                    if (f->off == WINDOW && warm && (f->end - c0 == 2 || f->end - c0 == 3)) ctr[CC_FIRST_FAR_LEN + (f->end - c0 - 2)]++;
                }
            }
            ctr[CC_BIT_AT_MOD32 + (r[CP_BIT_AT] & 31)]++;
            ctr[CC_NBITS_MOD32 + (r[CP_BITS] & 31)]++;
            if (r[CP_BITS] < 32) ctr[CC_UNDER_32]++;
            /* the 32-bit words of the stream this segment puts bits into: its first may be the last of the segments before */
            /* (word: that of the last bit so far; sharers: the segments with bits in it) */
            const uint64_t first_word = r[CP_BIT_AT] >> 5, last_word = (r[CP_BIT_AT] + r[CP_BITS] - 1) >> 5;
            if (first_word == word) {
                sharers++;
                if (last_full + 1 < k) ctr[CC_EMPTY_BETWEEN_SHARERS]++;
            } else
                sharers = 1;
            if (sharers > ctr[CC_WORD_SHARE_MAX]) ctr[CC_WORD_SHARE_MAX] = sharers;
            if (last_word != first_word) sharers = 1;
            word = last_word;
            last_full = k;
            if (r[CP_OVERSIZED]) {
                const uint64_t ph = r[CP_BIT_AT] & 2047;
                noversized++;
                ctr[CC_OVER_BIT_AT + (ph == 0 ? 0 : ph <= 31 ? 1 : ph >= 2017 ? 3 : 2)]++;
                if (k == 0) ctr[CC_OVER_SEG0]++;
                if (empties && k + 1 + empties < nseg && s[(k + 1 + empties) * CP_FIELDS + CP_TOKENS] == 1) ctr[CC_OVER_EMPTIES_ONE_TOKEN]++;
            }
        }
        if (noversized >= 2) ctr[CC_OVER_TWO]++;
        if (n) {
            const uint64_t *r = s + (nseg - 1) * CP_FIELDS;
            static const unsigned mods[5] = { 1, 63, 64, 255, 0 };
            ctr[CC_TOTAL_MOD32 + (bit & 31)]++;
            if (r[CP_EMPTY]) ctr[CC_MARKER_BEHIND_EMPTY]++;
            if (last_full < nseg && s[last_full * CP_FIELDS + CP_OVERSIZED]) ctr[CC_MARKER_BEHIND_OVERSIZED]++;
            for (int m = 0; m < 5; m++)
                if (n % seg == mods[m]) ctr[CC_LEN_MOD + m]++;
            /* the last token, and the one before it */
            size_t last = 0, before = 0;
            for (size_t c = 0; c < n; c = TOKEN(c)->end) { before = last; last = c; }
            const cp_tok_t *t = TOKEN(last);
            if (t->close == 0)  ctr[CC_END_CLOSE + 0]++;
            if (t->close == 14) ctr[CC_END_CLOSE + 1]++;
            if (!t->off && last && TOKEN(before)->off && last == n - 1) ctr[CC_END_ONE_SHORT]++;
        }
    }
    for (size_t k = 0; k < nseg && k < max_seg; k++)
        memcpy(rec + k * CP_FIELDS, s + k * CP_FIELDS, CP_FIELDS * sizeof(uint64_t));
#undef TOKEN
#undef SEG_END
done:
    free(memo); free(is_start); free(prev); free(head); free(s); free(entry); free(exitp); free(dirty);
    return result;
}

/* The sizes of what lzs_oracle_compress_segments fills in: counters, words a segment, kinds, columns of the last-token matrix. */
void lzs_oracle_compress_segments_layout(uint32_t *sizes)
{
    sizes[0] = CC_COUNTERS; sizes[1] = CP_FIELDS; sizes[2] = CK_KINDS; sizes[3] = CC_PAST;
}

/* The sizes of what lzs_oracle_scan_segments fills in: counters, words a segment, step kinds, columns of the straddle matrix. */
void lzs_oracle_scan_layout(uint32_t *sizes)
{
    sizes[0] = SC_COUNTERS; sizes[1] = SS_FIELDS; sizes[2] = SK_KINDS; sizes[3] = SC_B;
}
