/*
 * lzs_channels.c -- many channels, one packet each, and many packets per channel in one call (include/lzs/lzs_channels.h): the
 * arguments are checked here, the kernels (lzs_compress_channels_wg_kernel, lzs_decompress_channels_grp_kernel in lzs_kernels.hip;
 * lzs_channels_burst.hip) do the rest.
 */
#include "lzs_internal.h"
#include "lzs_burst_plan.h"
#include "lzs/lzs_channels.h"

_Static_assert(LZS_BURST_PACKETS_MAX == LZS_CHANNELS_MAX && LZS_BURST_SLOT_BYTES == LZS_CHANNEL_STATE_BYTES, "lzs_burst_plan.h is written for these");

typedef int (*channel_launch_fn)(void *, size_t, uint32_t, uint32_t *, const void *, size_t, const uint32_t *, uint32_t,
                                 const uint32_t *, void *, uint8_t *, uint32_t, void *);

/* a burst's checks, strided or packed: the ids and the work area */
int check_burst(const char *who, const uint32_t *d_channel, size_t nchannels, const void *d_work, size_t work_bytes, size_t npackets)
{
    if (!d_channel) return fail(LZS_E_ARG, "%s: channel is NULL", who);
    if (nchannels == 0) return fail(LZS_E_ARG, "%s: no channels for %zu packets", who, npackets);
    if (nchannels > LZS_CHANNELS_MAX) return fail(LZS_E_ARG, "%s: too many channels (%zu)", who, nchannels);
    if (!d_work) return fail(LZS_E_ARG, "%s: work is NULL", who);
    if ((uintptr_t)d_work & 255u) return fail(LZS_E_ARG, "%s: work is not 256-byte aligned", who);
    const size_t need = lzs_burst_plan_work_bytes(npackets, nchannels);
    if (work_bytes < need)
        return fail(LZS_E_ARG, "%s: work_bytes %zu is smaller than lzs_channels_burst_work_bytes() = %zu", who, work_bytes, need);
    return LZS_OK;
}

/* Every strided call's checks, in the order a call with several faults reports them: a burst's own have their place among them. */
static int check_strided(const char *who, int burst, const void *d_out, size_t out_cap, const uint32_t *d_out_len, const void *d_in,
                         const uint32_t *d_in_len, size_t in_len, const uint32_t *d_channel, const void *d_states, size_t nchannels,
                         const void *d_work, size_t work_bytes, size_t npackets)
{
    if (npackets > LZS_CHANNELS_MAX) return fail(LZS_E_ARG, "%s: too many packets (%zu)", who, npackets);
    if (!d_out_len) return fail(LZS_E_ARG, "%s: out_len is NULL", who);
    int rc = check_states(who, d_states);
    if (rc == LZS_OK && burst) rc = check_burst(who, d_channel, nchannels, d_work, work_bytes, npackets);
    if (rc != LZS_OK) return rc;
    if (!d_in && (in_len || d_in_len)) return fail(LZS_E_ARG, "%s: input is NULL", who);
    if (!d_out && out_cap) return fail(LZS_E_ARG, "%s: output is NULL", who);
    if (in_len > LZS_BLOCK_MAX) return fail(LZS_E_ARG, "%s: packet of %zu bytes exceeds LZS_BLOCK_MAX", who, in_len);
    if (d_in_len && (const void *)d_in_len == (const void *)d_out_len)
        return fail(LZS_E_ARG, "%s: d_out_len and d_in_len are the same array", who);
    return require_device();
}

static int device_channels(const char *who, channel_launch_fn launch, void *d_out, size_t out_stride, size_t out_cap,
                           uint32_t *d_out_len, const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                           const uint32_t *d_channel, void *d_states, uint8_t *d_status, size_t npackets, void *stream)
{
    if (npackets == 0) return LZS_OK;
    const int rc = check_strided(who, 0, d_out, out_cap, d_out_len, d_in, d_in_len, in_len, d_channel, d_states, 0, NULL, 0, npackets);
    if (rc != LZS_OK) return rc;
    const uint32_t cap32 = out_cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)out_cap;
    const int e = launch(d_out, out_stride, cap32, d_out_len, d_in, in_stride, d_in_len, (uint32_t)in_len, d_channel, d_states,
                         d_status, (uint32_t)npackets, stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

int lzs_compress_channels_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                 const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                 const uint32_t *d_channel, void *d_states, uint8_t *d_status,
                                 size_t npackets, void *hip_stream)
{
    return device_channels("lzs_compress_channels_device", lzs_hip_launch_compress_channels, d_out, out_stride, out_cap,
                           d_out_len, d_in, in_stride, d_in_len, in_len, d_channel, d_states, d_status, npackets, hip_stream);
}

/* The burst's work area and the strided decoder's larger one (lzs_burst_plan.h). */
size_t lzs_channels_burst_work_bytes(size_t npackets, size_t nchannels) { return lzs_burst_plan_work_bytes(npackets, nchannels); }
size_t lzs_channels_burst_split_work_bytes(size_t npackets, size_t nchannels, size_t out_cap) { return lzs_burst_plan_split_work_bytes(npackets, nchannels, out_cap); }

/* Many packets per channel (lzs_channels_burst.hip). */
static int device_burst(const char *who, int decompress, void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                        const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len, const uint32_t *d_channel,
                        const uint8_t *d_flags, void *d_states, size_t nchannels, uint8_t *d_status, void *d_work, size_t work_bytes, size_t npackets,
                        void *stream)
{
    if (npackets == 0) return LZS_OK;
    const int rc = check_strided(who, 1, d_out, out_cap, d_out_len, d_in, d_in_len, in_len, d_channel, d_states, nchannels, d_work, work_bytes, npackets);
    if (rc != LZS_OK) return rc;
    const uint32_t cap32 = out_cap > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)out_cap;
    /* the decoder may split long runs if the caller gave it the room for the origins */
    const lzs_burst_split_t split = lzs_burst_plan_split_strided(decompress, work_bytes, npackets, nchannels, cap32);
    const lzs_env_t *env = lzs_env();
    const int e = lzs_hip_burst(decompress, d_out, out_stride, cap32, d_out_len, d_in, in_stride, d_in_len, (uint32_t)in_len,
                                d_channel, d_flags, d_states, (uint32_t)nchannels, d_status, d_work, (uint32_t)npackets, split.split,
                                lzs_burst_plan_split_min(env->burst_split_set, env->burst_split_min), stream);
    return e ? hip_fail(e, who) : LZS_OK;
}

/* The burst entries are the flags entries without flags (lzs_channels.h, LZS_PACKET_RESET): one path, one set of checks. */
int lzs_compress_channels_burst_flags_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                             const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                             const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, size_t nchannels,
                                             uint8_t *d_status, void *d_work, size_t work_bytes, size_t npackets, void *hip_stream)
{
    return device_burst("lzs_compress_channels_burst_flags_device", 0, d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len,
                        in_len, d_channel, d_flags, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_decompress_channels_burst_flags_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                               const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                               const uint32_t *d_channel, const uint8_t *d_flags, void *d_states, size_t nchannels,
                                               uint8_t *d_status, void *d_work, size_t work_bytes, size_t npackets, void *hip_stream)
{
    return device_burst("lzs_decompress_channels_burst_flags_device", 1, d_out, out_stride, out_cap, d_out_len, d_in, in_stride,
                        d_in_len, in_len, d_channel, d_flags, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_compress_channels_burst_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                       const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                       const uint32_t *d_channel, void *d_states, size_t nchannels, uint8_t *d_status,
                                       void *d_work, size_t work_bytes, size_t npackets, void *hip_stream)
{
    return device_burst("lzs_compress_channels_burst_device", 0, d_out, out_stride, out_cap, d_out_len, d_in, in_stride, d_in_len,
                        in_len, d_channel, NULL, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_decompress_channels_burst_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                         const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                         const uint32_t *d_channel, void *d_states, size_t nchannels, uint8_t *d_status,
                                         void *d_work, size_t work_bytes, size_t npackets, void *hip_stream)
{
    return device_burst("lzs_decompress_channels_burst_device", 1, d_out, out_stride, out_cap, d_out_len, d_in, in_stride,
                        d_in_len, in_len, d_channel, NULL, d_states, nchannels, d_status, d_work, work_bytes, npackets, hip_stream);
}

int lzs_decompress_channels_device(void *d_out, size_t out_stride, size_t out_cap, uint32_t *d_out_len,
                                   const void *d_in, size_t in_stride, const uint32_t *d_in_len, size_t in_len,
                                   const uint32_t *d_channel, void *d_states, uint8_t *d_status,
                                   size_t npackets, void *hip_stream)
{
    return device_channels("lzs_decompress_channels_device", lzs_hip_launch_decompress_channels, d_out, out_stride, out_cap,
                           d_out_len, d_in, in_stride, d_in_len, in_len, d_channel, d_states, d_status, npackets, hip_stream);
}
