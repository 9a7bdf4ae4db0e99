// tests/cpu_shim/size_walk/driver.cc -- csrc/lzs_decoded_size.hip compiled as host C++ (hip/hip_runtime.h beside this file) and
// run under the address sanitizer (tests/test_decoded_size_host.py).  usage: driver CASES OUT
//   CASES: uint32 ncases, then per case uint32 n, uint32 offset, uint32 limit and n bytes
//   OUT  : per case uint32 size, uint32 status
// Every stream lies in an allocation of its own that begins `offset` bytes in front of it and ends with the aligned 32-bit word
// that holds its last byte (an empty stream: with nothing behind it), so a read outside the words that hold the stream's own
// bytes stops the run.  Every case is also run through the length array, without a status array, and between guard words.
#include "lzs_decoded_size.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t nc;
    if (!f || !o || fread(&nc, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < nc; c++) {
        uint32_t h[3];
        if (fread(h, 4, 3, f) != 3) return 2;
        const uint32_t n = h[0], a0 = h[1], limit = h[2];
        const size_t alloc = n ? (a0 + n + 3) / 4 * 4 : a0;
        uint8_t *buf = (uint8_t *)malloc(alloc ? alloc : 1);
        for (size_t i = 0; i < alloc; i++) buf[i] = (uint8_t)rand();
        if (n && fread(buf + a0, 1, n, f) != n) return 2;
        uint32_t size[3] = {0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu}, size2 = 0, len = n;
        uint8_t st[3] = {0xAA, 0xAA, 0xAA};
        int e = lzs_hip_launch_decoded_size(size + 1, st + 1, buf + a0, 0, (c & 1) ? &len : nullptr, (c & 1) ? 12345u : n, limit, 1,
                                            nullptr);
        e |= lzs_hip_launch_decoded_size(&size2, nullptr, buf + a0, 0, nullptr, n, limit, 1, nullptr);
        if (e || size[0] != 0xAAAAAAAAu || size[2] != 0xAAAAAAAAu || st[0] != 0xAA || st[2] != 0xAA || size2 != size[1]) {
            printf("case %u: guard words changed, or the sizes differ without a status array\n", c);
            return 1;
        }
        const uint32_t r[2] = {size[1], st[1]};
        fwrite(r, 4, 2, o);
        free(buf);
    }
    fclose(o);
    // batches: wavefront and grid tails, a stride that is no multiple of four
    for (uint32_t nb : {1u, 63u, 64u, 65u, 129u}) {
        std::vector<uint8_t> in(nb * 17u, 0);
        std::vector<uint32_t> size(nb + 2u, 7u), len(nb);
        for (uint32_t b = 0; b < nb; b++) { len[b] = b % 3u ? 2u : 0u; in[b * 17u] = 0xC0; }
        if (lzs_hip_launch_decoded_size(size.data() + 1, nullptr, in.data(), 17, len.data(), 0, 100, nb, nullptr)) return 1;
        if (size[0] != 7u || size[nb + 1u] != 7u) { printf("batch of %u: guard words changed\n", nb); return 1; }
        for (uint32_t b = 0; b < nb; b++) if (size[b + 1u] != 0u) { printf("batch of %u: block %u\n", nb, b); return 1; }
    }
    printf("ok %u cases\n", nc);
    return 0;
}
