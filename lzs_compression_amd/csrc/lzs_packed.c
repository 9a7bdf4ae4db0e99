/*
 * lzs_packed.c -- the offset-addressed ("packed") calls (include/lzs/lzs_batch.h, lzs_channels.h):
 * lzs_offsets_from_sizes_device, lzs_decompressed_size_packed_device, lzs_decompress_batch_packed_device,
 * lzs_decompress_channels_packed_device; lzs_compressed_bound_packed_device, lzs_compress_batch_packed_device,
 * lzs_compress_channels_packed_device, lzs_compact_packed_device; lzs_channels_burst_packed_split_work_bytes,
 * lzs_compress_channels_burst_packed_device, lzs_decompress_channels_burst_packed_device.  The arguments are checked here; lzs_scan_sizes_kernel,
 * lzs_decoded_size_packed_kernel (lzs_decoded_size.hip), lzs_decompress_packed_grp_kernel (kernels/decompress_packed.inc), the packed
 * entries of kernels/compress_wg.inc and compress_aux.inc and lzs_gather_packed_kernel (kernels/compact_resume.inc) do the rest.
 * Offsets and lengths stay on the device: what they say about a single block is the kernels' to check.
 */
#include "lzs_internal.h"
#include "lzs_burst_plan.h"
#include "lzs/lzs_channels.h"

static int offsets_aligned(const char *who, const char *name, const uint64_t *p)
{
    if ((uintptr_t)p & 7u) return fail(LZS_E_ARG, "%s: %s is not 8-byte aligned", who, name);
    return LZS_OK;
}

int lzs_offsets_from_sizes_device(uint64_t *d_offsets, const uint32_t *d_size, size_t align, size_t nblocks, void *hip_stream)
{
    const char *who = "lzs_offsets_from_sizes_device";
    if (!d_offsets) return fail(LZS_E_ARG, "%s: offsets is NULL", who);
    if (!d_size && nblocks) return fail(LZS_E_ARG, "%s: size is NULL", who);
    int rc = offsets_aligned(who, "d_offsets", d_offsets);
    if (rc != LZS_OK) return rc;
    if (align == 0 || align > 256u || (align & (align - 1u)) != 0)
        return fail(LZS_E_ARG, "%s: align %zu is not a power of two from 1 to 256", who, align);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_scan_sizes(d_offsets, d_size, (uint32_t)align, (uint32_t)nblocks, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

int lzs_decompressed_size_packed_device(uint32_t *d_size, uint8_t *d_status, const void *d_in, const uint64_t *d_in_off,
                                        const uint32_t *d_in_len, size_t limit, size_t nblocks, void *hip_stream)
{
    const char *who = "lzs_decompressed_size_packed_device";
    if (nblocks == 0) return LZS_OK;
    if (!d_size) return fail(LZS_E_ARG, "%s: size is NULL", who);
    if (!d_in) return fail(LZS_E_ARG, "%s: input is NULL", who);
    if (!d_in_off) return fail(LZS_E_ARG, "%s: in_off is NULL", who);
    int rc = offsets_aligned(who, "d_in_off", d_in_off);
    if (rc != LZS_OK) return rc;
    if (d_in_len && (const void *)d_in_len == (const void *)d_size)
        return fail(LZS_E_ARG, "%s: d_size and d_in_len are the same array", who);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    if (limit > 0xFFFFFFFFu) return fail(LZS_E_ARG, "%s: limit %zu exceeds 0xFFFFFFFF", who, limit);
    rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_decoded_size_packed(d_size, d_status, d_in, d_in_off, d_in_len, (uint32_t)limit, (uint32_t)nblocks,
                                                     hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

/* what the decoders and the compressors ask of their arguments */
static int check_decode(const char *who, const void *d_out, const uint64_t *d_out_off, const uint32_t *d_out_len, const void *d_in,
                        const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks)
{
    if (!d_out) return fail(LZS_E_ARG, "%s: output is NULL", who);
    if (!d_out_off) return fail(LZS_E_ARG, "%s: out_off is NULL", who);
    if (!d_out_len) return fail(LZS_E_ARG, "%s: out_len is NULL", who);
    if (!d_in) return fail(LZS_E_ARG, "%s: input is NULL", who);
    if (!d_in_off) return fail(LZS_E_ARG, "%s: in_off is NULL", who);
    int rc = offsets_aligned(who, "d_out_off", d_out_off);
    if (rc != LZS_OK) return rc;
    rc = offsets_aligned(who, "d_in_off", d_in_off);
    if (rc != LZS_OK) return rc;
    if (d_in_len && (const void *)d_in_len == (const void *)d_out_len)
        return fail(LZS_E_ARG, "%s: d_out_len and d_in_len are the same array", who);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    return LZS_OK;
}

int lzs_decompress_batch_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                       const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks, void *hip_stream)
{
    const char *who = "lzs_decompress_batch_packed_device";
    if (nblocks == 0) return LZS_OK;
    int rc = check_decode(who, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, nblocks);
    if (rc != LZS_OK) return rc;
    rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_decompress_packed(d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, (uint32_t)nblocks, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

int lzs_decompress_channels_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                          const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                          void *d_states, uint8_t *d_status, size_t npackets, void *hip_stream)
{
    const char *who = "lzs_decompress_channels_packed_device";
    if (npackets == 0) return LZS_OK;
    int rc = check_decode(who, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, npackets);
    if (rc == LZS_OK) rc = check_states(who, d_states);
    if (rc == LZS_OK) rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_decompress_channels_packed(d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, d_channel, d_states,
                                                            d_status, (uint32_t)npackets, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

int lzs_compressed_bound_packed_device(uint32_t *d_bound, const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks,
                                       void *hip_stream)
{
    const char *who = "lzs_compressed_bound_packed_device";
    if (nblocks == 0) return LZS_OK;
    if (!d_bound) return fail(LZS_E_ARG, "%s: bound is NULL", who);
    if (!d_in_off) return fail(LZS_E_ARG, "%s: in_off is NULL", who);
    int rc = offsets_aligned(who, "d_in_off", d_in_off);
    if (rc != LZS_OK) return rc;
    if (d_in_len && (const void *)d_in_len == (const void *)d_bound)
        return fail(LZS_E_ARG, "%s: d_bound and d_in_len are the same array", who);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_compressed_bound_packed(d_bound, d_in_off, d_in_len, (uint32_t)nblocks, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

int lzs_compress_batch_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                     const uint64_t *d_in_off, const uint32_t *d_in_len, size_t nblocks, void *hip_stream)
{
    const char *who = "lzs_compress_batch_packed_device";
    if (nblocks == 0) return LZS_OK;
    int rc = check_decode(who, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, nblocks);
    if (rc != LZS_OK) return rc;
    rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_compress_packed(d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, (uint32_t)nblocks, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

int lzs_compress_channels_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                        const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                        void *d_states, uint8_t *d_status, size_t npackets, void *hip_stream)
{
    const char *who = "lzs_compress_channels_packed_device";
    if (npackets == 0) return LZS_OK;
    int rc = check_decode(who, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, npackets);
    if (rc == LZS_OK) rc = check_states(who, d_states);
    if (rc == LZS_OK) rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_compress_channels_packed(d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, d_channel, d_states,
                                                          d_status, (uint32_t)npackets, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

/* Packed bursts (lzs_channels_burst.hip): the checks of the packed calls above and a burst's (check_burst).  What the
 * work area holds behind the burst size is room for origins (lzs_burst_plan.h): whether the rooms fit it is the device's to see
 * (lzs_burst_split_plan_packed_kernel). */
size_t lzs_channels_burst_packed_split_work_bytes(size_t npackets, size_t nchannels, uint64_t out_bytes)
{
    return lzs_burst_plan_packed_split_work_bytes(npackets, nchannels, out_bytes);
}

static int device_burst_packed(const char *who, int decompress, void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len,
                               const void *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                               const uint8_t *d_flags, void *d_states, size_t nchannels, uint8_t *d_status, void *d_work,
                               size_t work_bytes, size_t npackets, void *stream)
{
    if (npackets == 0) return LZS_OK;
    int rc = check_decode(who, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, npackets);
    if (rc == LZS_OK) rc = check_states(who, d_states);
    if (rc == LZS_OK) rc = check_burst(who, d_channel, nchannels, d_work, work_bytes, npackets);
    if (rc == LZS_OK) rc = require_device();
    if (rc != LZS_OK) return rc;
    const lzs_burst_split_t split = lzs_burst_plan_split_packed(decompress, work_bytes - lzs_burst_plan_work_bytes(npackets, nchannels));
    const lzs_env_t *env = lzs_env();
    const int e = lzs_hip_burst_packed(decompress, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len, d_channel, d_flags, d_states,
                                       (uint32_t)nchannels, d_status, d_work, (uint32_t)npackets, split.split, split.origin_cap,
                                       lzs_burst_plan_split_min(env->burst_split_set, env->burst_split_min), stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

/* The packed burst entries are the flags entries without flags (lzs_channels.h, LZS_PACKET_RESET). */
int lzs_compress_channels_burst_packed_flags_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                                    const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                                    const uint8_t *d_flags, void *d_states, size_t nchannels, uint8_t *d_status,
                                                    void *d_work, size_t work_bytes, size_t npackets, void *hip_stream)
{
    return device_burst_packed("lzs_compress_channels_burst_packed_flags_device", 0, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len,
                               d_channel, d_flags, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_decompress_channels_burst_packed_flags_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                                      const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                                      const uint8_t *d_flags, void *d_states, size_t nchannels, uint8_t *d_status,
                                                      void *d_work, size_t work_bytes, size_t npackets, void *hip_stream)
{
    return device_burst_packed("lzs_decompress_channels_burst_packed_flags_device", 1, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len,
                               d_channel, d_flags, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_compress_channels_burst_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                              const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                              void *d_states, size_t nchannels, uint8_t *d_status, void *d_work, size_t work_bytes,
                                              size_t npackets, void *hip_stream)
{
    return device_burst_packed("lzs_compress_channels_burst_packed_device", 0, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len,
                               d_channel, NULL, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_decompress_channels_burst_packed_device(void *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, const void *d_in,
                                                const uint64_t *d_in_off, const uint32_t *d_in_len, const uint32_t *d_channel,
                                                void *d_states, size_t nchannels, uint8_t *d_status, void *d_work, size_t work_bytes,
                                                size_t npackets, void *hip_stream)
{
    return device_burst_packed("lzs_decompress_channels_burst_packed_device", 1, d_out, d_out_off, d_out_len, d_in, d_in_off, d_in_len,
                               d_channel, NULL, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_compact_packed_device(void *d_dense, uint64_t *d_offsets, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_len,
                              size_t nblocks, void *hip_stream)
{
    const char *who = "lzs_compact_packed_device";
    if (nblocks == 0) return LZS_OK;
    if (!d_dense) return fail(LZS_E_ARG, "%s: dense is NULL", who);
    if (!d_offsets) return fail(LZS_E_ARG, "%s: offsets is NULL", who);
    if (!d_src) return fail(LZS_E_ARG, "%s: src is NULL", who);
    if (!d_src_off) return fail(LZS_E_ARG, "%s: src_off is NULL", who);
    if (!d_len) return fail(LZS_E_ARG, "%s: len is NULL", who);
    int rc = offsets_aligned(who, "d_offsets", d_offsets);
    if (rc != LZS_OK) return rc;
    rc = offsets_aligned(who, "d_src_off", d_src_off);
    if (rc != LZS_OK) return rc;
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_compact_packed(d_dense, d_offsets, d_src, d_src_off, d_len, (uint32_t)nblocks, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}
