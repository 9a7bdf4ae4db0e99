/*
 * lzs/lzs_channels.h -- additive entry points of the MI355X build of liblzs: many channels, one packet each, per launch.
 *
 * A channel is one LZS history carried from packet to packet, the "sequential history" of RFC 1974: a packet may refer back
 * into the packets before it on the same channel.  The reference keeps such a history in one parameter block per stream
 * (lzs_compress_incremental() / lzs_decompress_incremental(), lzs.h), one call per packet.  The calls below take thousands of
 * channels in one launch -- the shape of a PPP or tunnel endpoint that holds one history per link or session.
 *
 * CHANNEL STATE.  A channel is an opaque slot of LZS_CHANNEL_STATE_BYTES bytes in device memory, 4-byte aligned:
 *
 *     offset 0   uint32_t hist_len         bytes of history, 0 .. 2047
 *     offset 4   reserved, zero            (to offset 64)
 *     offset 64  uint8_t  hist[2048]       hist[0 .. hist_len): the history, oldest byte first; the rest zero
 *
 * An all-zero slot is a new channel: lzs_compress_init_full() for the compressor, lzs_decompress_init() for the
 * decompressor.  Setting hist_len to 0 resets a channel.  Compressor and decompressor states have the same layout but are
 * separate arrays; after a packet that went through both cleanly, the compressor's slot and the peer decompressor's slot hold
 * the same bytes (both calls rewrite all of hist[]: the history, then zeros).
 *
 * All functions return LZS_OK (0) or a negative LZS_E_* code (lzs_batch.h); lzs_last_error() gives the message.
 */
#ifndef LZS_MI355X_LZS_CHANNELS_H
#define LZS_MI355X_LZS_CHANNELS_H

#include <stddef.h>
#include <stdint.h>

#include "lzs_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LZS_CHANNEL_STATE_BYTES  2112u   /* one channel's slot: 64-byte header + 2048 bytes of history */
#define LZS_CHANNEL_HISTORY_AT   64u     /* offset of hist[] in a slot */
#define LZS_CHANNELS_MAX         0x7FFFFFFFu   /* packets per call */

/*
 * Device-pointer channel compression, asynchronous on `hip_stream`.
 *
 *   packet b input  : d_in  + b * in_stride,  length d_in_len ? d_in_len[b] : in_len (at most LZS_BLOCK_MAX)
 *   packet b output : d_out + b * out_stride, capacity out_cap;  d_out_len[b]: bytes written
 *   packet b channel: c = d_channel ? d_channel[b] : b;  its state: d_states + c * LZS_CHANNEL_STATE_BYTES
 *
 * Packet b's bytes are what lzs_compress_incremental(&P_c, true) writes when P_c was initialised and fed the channel's earlier
 * packets the same way, and the packet is given whole with room for LZS_COMPRESSED_MAX(len) bytes: a stream that starts at
 * bit 0 and ends with the end marker and its padding, whose matches may reach back into the channel's history.  Afterwards
 * the channel's history is the last min(2047, hist_len + len) bytes of history | packet.
 *
 * d_status[b] (d_status may be NULL) receives the reference's LZS_C_STATUS_* bits: END_MARKER | INPUT_FINISHED |
 * INPUT_STARVED for a whole packet.  If out_cap is too small the output is cut there, as lzs_compress() cuts it; the history
 * still advances, and the status has NO_OUTPUT_BUFFER_SPACE instead of END_MARKER -- the peer cannot follow, so reset the
 * channel.  A slot with hist_len > 2047 is not a state: that packet gets ERROR and d_out_len[b] = 0, and nothing else of it
 * is written or changed.
 *
 * A CHANNEL MAY APPEAR AT MOST ONCE PER CALL (packets of one channel depend on each other: give them in successive calls, or
 * in one call of the burst entries below).  If one repeats, what that channel's packets and state receive is undefined; the
 * other channels are not affected.
 *
 * Arguments are checked before the device is asked (LZS_E_ARG): d_states and d_out_len must be given, d_states 4-byte
 * aligned, d_out_len must not be the array d_in_len, npackets at most LZS_CHANNELS_MAX.  Without a device a valid call
 * returns LZS_E_NO_DEVICE.  No allocation, no synchronisation: safe to capture into a hipGraph -- with the caveat of the
 * batch calls of lzs_batch.h: once per device and process the library asks the device how it orders same-address LDS
 * exchanges (a 0.1 ms kernel on a stream of its own, at the first entry into the library on that device, which allocates and
 * waits; `hip_stream` is not touched by it).  Call lzs_backend_info() first if the very first call is to be captured.
 */
int lzs_compress_channels_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                 const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                 const uint32_t *d_channel, void *d_states, uint8_t *d_status,
                                 size_t npackets, void *hip_stream);

/*
 * Device-pointer channel decompression: the same arguments, LZS_D_STATUS_* bits.  Each packet is decoded until its first end
 * marker, the end of its bytes or out_cap, with copies reaching into the channel's history; for a well-formed packet the
 * output is what lzs_decompress_incremental() gives on that channel's parameter block.  Bytes after the end marker are
 * ignored.  Status: END_MARKER; NO_OUTPUT_BUFFER_SPACE when out_cap stopped it first (also when a copy was cut at out_cap,
 * whatever follows it: the output is not the packet's, so reset the channel); INPUT_STARVED | INPUT_FINISHED when the bits
 * ran out first.  Afterwards the channel's history is the last min(2047, hist_len + produced) bytes of history | output.
 * A slot with hist_len > 2047 gets ERROR and d_out_len[b] = 0, as above.
 *
 * Differences from the reference: a packet that stops early keeps no partial token -- only the history carries over (RFC 1974
 * packets are whole).  An offset reaching before the channel's history reads zeros; a long offset of 0 follows the rule of
 * lzs_decompress_batch_device.  Malformed input never makes a packet read or write outside its own slots
 * and its channel's state.
 *
 * SIZING THE OUTPUT.  lzs_decompressed_size_batch_device() (lzs_batch.h) applies unchanged to channel and burst packets: give
 * it the packets (d_in, in_stride, d_in_len, in_len, npackets as here) and a limit, and it reports for every packet the
 * d_out_len[b] and d_status[b] this call and the burst call below would write with out_cap = limit on a valid channel,
 * whatever the channel's history -- a packet's length does not depend on the bytes it copies.  With limit = 0xFFFFFFFF these
 * are the packets' true sizes: what out_cap, or an output tensor, has to hold before lzs_decompress_channels*_device is
 * called.  It sees no slot, so it never reports ERROR and changes no history.
 */
int lzs_decompress_channels_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                   const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                   const uint32_t *d_channel, void *d_states, uint8_t *d_status,
                                   size_t npackets, void *hip_stream);

/*
 * lzs_decompress_channels_device() from PACKED packets to packed outputs: packet b lies at d_in + d_in_off[b] and is decoded to
 * d_out + d_out_off[b] with d_out_off[b + 1] - d_out_off[b] bytes of room -- the addressing, the containment, the entries that
 * are not a block (ERROR, d_out_len[b] = 0, the channel's slot untouched) and the argument checks are those of "PACKED streams"
 * in lzs_batch.h; d_states must be given and 4-byte aligned.  One packet per channel per call: the rule on repeated channels
 * above holds.  Every packet's bytes, d_out_len[b], d_status[b] and its channel's slot are byte for byte what
 * lzs_decompress_channels_device() gives for that packet alone with out_cap = its room; a slot with hist_len > 2047 gets ERROR
 * and d_out_len[b] = 0 as there.  lzs_decompressed_size_packed_device() sizes the rooms.  Many packets per channel:
 * lzs_decompress_channels_burst_packed_device() below.
 */
int lzs_decompress_channels_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                          const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                          void *d_states, uint8_t *d_status, size_t npackets, void *hip_stream);

/*
 * lzs_compress_channels_device() from PACKED packets to packed rooms: packet b lies at d_in + d_in_off[b] and is
 * compressed to d_out + d_out_off[b] with d_out_off[b + 1] - d_out_off[b] bytes of room, its out_cap -- addressing, containment,
 * entries that are not a block and argument checks as for "PACKED streams" and "PACKED COMPRESSION" in lzs_batch.h; d_states must be
 * given and 4-byte aligned.  One packet per channel per call.  Every packet's bytes, d_out_len[b], d_status[b] (END_MARKER |
 * INPUT_FINISHED | INPUT_STARVED = 0x07, or 0x0B with NO_OUTPUT_BUFFER_SPACE in END_MARKER's place where the room cut it) and its
 * channel's whole slot are those of lzs_compress_channels_device() for that packet alone with out_cap = its room.  A slot with
 * hist_len > 2047 gets ERROR and d_out_len[b] = 0, nothing changed; an entry that is not a block gets ERROR and d_out_len[b] = 0 and
 * its channel's slot is not touched.  lzs_compressed_bound_packed_device() sizes the rooms.  Many packets per channel:
 * lzs_compress_channels_burst_packed_device() below.
 */
int lzs_compress_channels_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                        const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                        void *d_states, uint8_t *d_status, size_t npackets, void *hip_stream);

/*
 * BURSTS: many packets per channel in one call -- a queue drained as it stands, busy links with many packets, most with none.
 *
 * The arguments are those of the calls above, and three more: nchannels (the slots in d_states), and a device work area
 * d_work of work_bytes bytes, 256-byte aligned, at least lzs_channels_burst_work_bytes(npackets, nchannels).  Both burst calls
 * take the same size: a little over one channel slot a packet.
 *
 * REPEATS ALLOWED.  d_channel (required here) may name a channel any number of times; the packets of one channel are taken in
 * ascending b.  Every packet's d_out bytes, d_out_len and d_status, and every channel's final slot, are byte for byte what
 * this gives: split the call into ranks (rank k = the k-th packet of every channel) and make one call of
 * lzs_compress_channels_device / lzs_decompress_channels_device per rank, in order.  So the rules above hold packet by
 * packet: a compressed packet cut at out_cap still advances its channel's history, a decoder copy cut at out_cap keeps
 * NO_OUTPUT_BUFFER_SPACE, and a channel whose slot has hist_len > 2047 gives ERROR and d_out_len[b] = 0 for every one of its
 * packets and keeps its slot untouched.  In addition d_channel[b] >= nchannels gives that packet ERROR and d_out_len[b] = 0.
 *
 * Arguments are checked before the device is asked (LZS_E_ARG), as above, and: d_channel and d_work must be given, d_work
 * 256-byte aligned, work_bytes no smaller than the size above, nchannels not 0 when there are packets and at most
 * LZS_CHANNELS_MAX.  No allocation and no synchronisation (the work area holds all scratch): safe to capture into a hipGraph,
 * with the caveat of the calls above.  A work area serves one call at a time.  Compression runs all packets in parallel
 * (each packet's history is input: the last 2047 bytes of its channel's slot and of the channel's packets before it);
 * decompression decodes each channel's packets in order, one decoder stream a channel, the channels with the most
 * compressed bytes first.
 *
 * LONG RUNS.  One decoder stream a channel makes the busiest channel the decoder's time.  A work area of at least
 * lzs_channels_burst_split_work_bytes(npackets, nchannels, out_cap) bytes -- the burst size plus about two bytes per packet and
 * byte of out_cap; SIZE_MAX where that does not fit a size_t -- lets lzs_decompress_channels_burst_device decode the packets of
 * long runs all at once and settle what they copy from each other afterwards.  The results are the same byte
 * for byte with either size of work area: d_out up to each d_out_len[b] and nothing past it, d_out_len, d_status, the slots.
 * The compressor ignores the extra room.
 */
size_t lzs_channels_burst_work_bytes(size_t npackets, size_t nchannels);
size_t lzs_channels_burst_split_work_bytes(size_t npackets, size_t nchannels, size_t out_cap);

int lzs_compress_channels_burst_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                       const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                       const uint32_t *d_channel, void *d_states, size_t nchannels, uint8_t *d_status,
                                       void *d_work, size_t work_bytes, size_t npackets, void *hip_stream);

int lzs_decompress_channels_burst_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                         const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                         const uint32_t *d_channel, void *d_states, size_t nchannels, uint8_t *d_status,
                                         void *d_work, size_t work_bytes, size_t npackets, void *hip_stream);

/*
 * PACKED BURSTS: a drained queue compressed or decoded where it lies -- many packets per channel, as in the burst
 * calls above, each addressed as in the packed calls: packet b lies at d_in + d_in_off[b] (d_in_len[b] bytes, or up to d_in_off[b + 1]
 * with d_in_len NULL) and goes to d_out + d_out_off[b] with d_out_off[b + 1] - d_out_off[b] bytes of room, clamped to 0xFFFFFFFF;
 * npackets + 1 output offsets are always read.  Addressing, containment -- a packet stores to [d_out_off[b], d_out_off[b] +
 * d_out_len[b]) of d_out and to no other byte of it -- and the entries that are not a block (offsets that decrease, a length above
 * LZS_BLOCK_MAX) are those of "PACKED streams" in lzs_batch.h.
 *
 * THE RESULT is the burst rule applied to the packed calls: split the call into ranks (rank k = the k-th packet of every channel, in
 * ascending b) and make one call of lzs_compress_channels_packed_device / lzs_decompress_channels_packed_device per rank, in order;
 * every packet's bytes, d_out_len[b] and d_status[b] and every channel's final slot are byte for byte what that gives.  So:
 *   - an entry that is not a block gets ERROR and d_out_len[b] = 0; nothing of it is read or written, it adds nothing to its
 *     channel's history, and the run goes on behind it with the history it had;
 *   - a channel whose packets in this call are all not blocks keeps its slot untouched byte for byte, whatever lies behind hist_len;
 *   - a slot with hist_len > 2047 gives every packet of that channel ERROR and d_out_len[b] = 0 and stays untouched, and so does
 *     d_channel[b] >= nchannels for that packet;
 *   - a compressed packet cut at its room has NO_OUTPUT_BUFFER_SPACE in END_MARKER's place (0x0B) and still advances the history; a
 *     decoder copy cut at its room gives NO_OUTPUT_BUFFER_SPACE and advances the history by what was produced;
 *   - a packet of no bytes is a block: the compressor writes its end marker, the history is as it was.
 *
 * SIZING THE ROOMS.  lzs_compressed_bound_packed_device() and lzs_decompressed_size_packed_device() (lzs_batch.h) apply unchanged: a
 * packet's compressed bound depends on its length alone, and its decoded length and status never depend on its channel's history.
 *
 * THE WORK AREA is that of the burst calls: d_work 256-byte aligned, work_bytes at least lzs_channels_burst_work_bytes(npackets,
 * nchannels), for both calls.  With at least lzs_channels_burst_packed_split_work_bytes(npackets, nchannels, out_bytes) bytes -- the
 * burst size plus two bytes per byte of room, out_bytes being the sum of the rooms (d_out_off[npackets] - d_out_off[0] for offsets
 * that ascend); SIZE_MAX where that does not fit a size_t -- the decoder may split long runs as above.  The offsets are on the device,
 * so the device decides: if the sum of the (clamped) rooms does not fit what the work area holds behind the burst size, no run of that
 * call is split.  The results are the same byte for byte whichever way a run is decoded, and nothing is written outside work_bytes.
 * The compressor ignores the extra room.
 *
 * Arguments are checked before the device is asked (LZS_E_ARG): those of the packed calls -- d_out, d_in, d_out_off, d_in_off and
 * d_out_len given, the offset arrays 8-byte aligned, d_out_len not the array d_in_len, npackets at most LZS_CHANNELS_MAX -- and those
 * of the burst calls -- d_states given and 4-byte aligned, d_channel and d_work given, d_work 256-byte aligned, work_bytes no smaller
 * than the burst size, nchannels not 0 when there are packets and at most LZS_CHANNELS_MAX.  npackets == 0 is LZS_OK and touches
 * nothing; without a device a valid call returns LZS_E_NO_DEVICE.  No allocation and no synchronisation: safe to capture into a
 * hipGraph, with the caveat of the calls above.
 */
size_t lzs_channels_burst_packed_split_work_bytes(size_t npackets, size_t nchannels, uint64_t out_bytes);

int lzs_compress_channels_burst_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len,
                                              const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                              const uint32_t *d_channel, void *d_states, size_t nchannels, uint8_t *d_status,
                                              void *d_work, size_t work_bytes, size_t npackets, void *hip_stream);

int lzs_decompress_channels_burst_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len,
                                                const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                                const uint32_t *d_channel, void *d_states, size_t nchannels, uint8_t *d_status,
                                                void *d_work, size_t work_bytes, size_t npackets, void *hip_stream);

/*
 * HISTORY RESETS INSIDE A QUEUE.  RFC 1974 resets a link's history after a Reset-Request / Reset-Ack exchange or a
 * lost packet, and IPComp-style traffic (RFC 2395) does so in front of every packet.  Setting hist_len to 0 does that between calls;
 * the four entries below do it inside a burst.  Each takes the arguments of the burst entry it is named after and, directly behind
 * d_channel, d_flags: a device array of npackets bytes, or NULL.  Only bit 0, LZS_PACKET_RESET, is read; d_flags needs no alignment.
 *
 * With d_flags == NULL an entry is the burst entry it extends, byte for byte (the four burst entries above are these with NULL).
 *
 * THE RULE is the rank rule of the bursts, extended.  Split the call into ranks, rank k being the k-th packet of every channel in
 * ascending b, and make one call of lzs_*_channels_device (packed: lzs_*_channels_packed_device) per rank, in order.  Before the
 * call of rank k, for every packet of that rank that has LZS_PACKET_RESET set, whose channel id is below nchannels and (packed)
 * whose entry is a block, store 0 to its channel's hist_len.  Every packet's bytes, d_out_len[b], d_status[b] and every channel's
 * final slot are byte for byte what that sequence gives.  So:
 *   - a flagged packet is compressed, or decoded, from an empty history, whatever the slot or the packets before it held; in the
 *     decoder an offset that reaches in front of the flagged packet's own output reads zeros;
 *   - a flag on the first packet of a channel discards the slot's history;
 *   - a slot with hist_len > 2047 gives ERROR to the channel's packets before its first flagged block; from that block on the
 *     channel is a valid, empty one, and it ends the call with a canonical slot (hist_len, the history, zeros behind it);
 *   - a flag on an id >= nchannels is ignored: that packet gets ERROR as without it;
 *   - a flag on a packed entry that is not a block is ignored: the entry does nothing at all, and the run goes on behind it with the
 *     history it had;
 *   - a flagged packet of no bytes leaves its channel with hist_len 0 and hist[] all zero (until the next packet), and so does a
 *     flagged decoder packet that produces nothing;
 *   - a compressed packet cut at its room, or a decoder copy cut at its room, behaves as without flags: a flag changes only the
 *     history the packet starts from.
 *
 * A flagged packet depends on nothing in front of it, so the decoder treats it as the start of a new run: a queue of one channel
 * in which every packet is flagged decodes like a batch of independent blocks, not like one long run.
 *
 * The work areas are those of the burst entries, unchanged in size: lzs_channels_burst_work_bytes(), and for the decoder's split
 * lzs_channels_burst_split_work_bytes() / lzs_channels_burst_packed_split_work_bytes().  The argument checks are those of the burst
 * entries, with the entry's own name in lzs_last_error(); npackets == 0 is LZS_OK and touches nothing; without a device a valid call
 * returns LZS_E_NO_DEVICE.  Asynchronous on hip_stream, no allocation, no synchronisation: safe to capture into a hipGraph, with the
 * caveat of the calls above.
 */
#define LZS_PACKET_RESET 0x01u   /* d_flags[b]: reset the channel's history in front of packet b */

int lzs_compress_channels_burst_flags_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                             const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                             const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, size_t nchannels,
                                             uint8_t *d_status, void *d_work, size_t work_bytes, size_t npackets, void *hip_stream);

int lzs_decompress_channels_burst_flags_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                               const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                               const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, size_t nchannels,
                                               uint8_t *d_status, void *d_work, size_t work_bytes, size_t npackets, void *hip_stream);

int lzs_compress_channels_burst_packed_flags_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len,
                                                    const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                                    const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, size_t nchannels,
                                                    uint8_t *d_status, void *d_work, size_t work_bytes, size_t npackets,
                                                    void *hip_stream);

int lzs_decompress_channels_burst_packed_flags_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len,
                                                      const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                                      const uint32_t *d_channel, const uint8_t *d_flags, void *d_states,
                                                      size_t nchannels, uint8_t *d_status, void *d_work, size_t work_bytes,
                                                      size_t npackets, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* LZS_MI355X_LZS_CHANNELS_H */
