/*
 * lzs_size_query.c -- lzs_decompressed_size_batch_device (include/lzs/lzs_batch.h): the arguments are checked here, the token
 * walk is lzs_decoded_size_kernel (lzs_decoded_size.hip).
 */
#include "lzs_internal.h"

int lzs_decompressed_size_batch_device(uint32_t *d_size, uint8_t *d_status, const void *d_in, size_t in_stride,
                                       const uint32_t *d_in_len, size_t in_len, size_t limit, size_t nblocks, void *hip_stream)
{
    const char *who = "lzs_decompressed_size_batch_device";
    if (nblocks == 0) return LZS_OK;
    if (!d_size) return fail(LZS_E_ARG, "%s: size is NULL", who);
    if (!d_in) return fail(LZS_E_ARG, "%s: input is NULL", who);
    if (in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: block of %zu bytes exceeds LZS_BLOCK_MAX", who, in_len);
    if (nblocks > 0x7FFFFFFFu) return fail(LZS_E_ARG, "%s: too many blocks (%zu)", who, nblocks);
    if (limit > 0xFFFFFFFFu) return fail(LZS_E_ARG, "%s: limit %zu exceeds 0xFFFFFFFF", who, limit);
    /* (the lengths read are not the sizes written: a block's size may land before another wavefront has read its length) */
    if (d_in_len && (const void *)d_in_len == (const void *)d_size)
        return fail(LZS_E_ARG, "%s: d_size and d_in_len are the same array", who);
    int rc = require_device();
    if (rc != LZS_OK) return rc;
    const int e = lzs_hip_launch_decoded_size(d_size, d_status, d_in, in_stride, d_in_len, (uint32_t)in_len, (uint32_t)limit,
                                              (uint32_t)nblocks, hip_stream);
    return e ? hip_fail(e, who) : LZS_OK;
}
