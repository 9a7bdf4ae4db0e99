/*
 * oracle/lzs_oracle.c -- CPU restatement of the LZS one-shot codec, and plain models of one channel packet's decoding and
 * compression (lzs_oracle_decompress_channel, lzs_oracle_compress_channel: tests/test_channel_model.py,
 * tests/test_channel_encode_model.py hold them to the reference), and of what a segment border of the many-wavefront stream
 * decoders is (lzs_oracle_scan_segments: tests/test_stream_border_model.py).
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

/* The sizes of what lzs_oracle_scan_segments fills in: counters, words a segment, step kinds, columns of the straddle matrix. */
void lzs_oracle_scan_layout(uint32_t *sizes)
{
    sizes[0] = SC_COUNTERS; sizes[1] = SS_FIELDS; sizes[2] = SK_KINDS; sizes[3] = SC_B;
}
