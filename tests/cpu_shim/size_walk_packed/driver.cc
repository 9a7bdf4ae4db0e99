// tests/cpu_shim/size_walk_packed/driver.cc -- the packed size kernel of csrc/lzs_decoded_size.hip compiled as host C++ (the stub
// ../size_walk/hip/hip_runtime.h, by include path) and run under the address and undefined-behaviour sanitizers
// (tests/test_packed_size_host.py).  usage: driver CASES OUT
//   CASES: uint32 nbatches, then per batch uint32 limit, uint32 nb and per entry uint32 n, uint32 a0, uint32 kind and n bytes
//   OUT  : per entry uint32 size, status of the batched call with lengths, then size, status of a call without lengths
// Every stream lies in an allocation of its own that begins a0 bytes in front of it and ends with the aligned 32-bit word that
// holds its last byte (an empty stream: with nothing behind it), so a read outside the words that hold the stream's own bytes
// stops the run.  d_in is the lowest of those allocations, the offsets are the distances from it -- in whatever order malloc
// and the batch's (shuffled) order give.  A batch is one call with d_in_len; then every entry once more without lengths, as the
// pair {from, from + n}.  kind 1: with lengths the entry's length is LZS_BLOCK_MAX + 1; kind 2: without lengths its pair decreases
// -- neither is a block, and its allocation is freed before the call, so that a read of it stops the run.
#include "lzs_decoded_size.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t nbatches, total = 0;
    if (!f || !o || fread(&nbatches, 4, 1, f) != 1) return 2;
    for (uint32_t t = 0; t < nbatches; t++) {
        uint32_t h[2];
        if (fread(h, 4, 2, f) != 2) return 2;
        const uint32_t limit = h[0], nb = h[1];
        std::vector<uint8_t *> buf(nb);
        std::vector<std::vector<uint8_t>> keep(nb);
        std::vector<uint32_t> n(nb), a0(nb), kind(nb);
        for (uint32_t b = 0; b < nb; b++) {
            uint32_t e[3];
            if (fread(e, 4, 3, f) != 3) return 2;
            n[b] = e[0]; a0[b] = e[1]; kind[b] = e[2];
            const size_t alloc = n[b] ? (a0[b] + n[b] + 3) / 4 * 4 : a0[b];
            buf[b] = (uint8_t *)malloc(alloc ? alloc : 1);
            for (size_t i = 0; i < alloc; i++) buf[b][i] = (uint8_t)rand();
            if (n[b] && fread(buf[b] + a0[b], 1, n[b], f) != n[b]) return 2;
            keep[b].assign(buf[b], buf[b] + alloc);
        }
        uintptr_t base = ~(uintptr_t)0;
        for (uint32_t b = 0; b < nb; b++) base = (uintptr_t)buf[b] < base ? (uintptr_t)buf[b] : base;
        const uint8_t *d_in = (const uint8_t *)base;
        std::vector<uint64_t> off(nb + 1, 0);
        std::vector<uint32_t> len(nb), size(nb + 2, 0xAAAAAAAAu);
        std::vector<uint8_t> st(nb + 2, 0xAA);
        for (uint32_t b = 0; b < nb; b++) {
            off[b] = (uint64_t)((uintptr_t)(buf[b] + a0[b]) - base);
            len[b] = kind[b] == 1 ? (3u << 30) + 1u : n[b];
            if (kind[b] == 1) { free(buf[b]); buf[b] = nullptr; }   // not a block: nothing of it may be read
        }
        if (lzs_hip_launch_decoded_size_packed(size.data() + 1, st.data() + 1, d_in, off.data(), len.data(), limit, nb, nullptr)) return 1;
        if (size[0] != 0xAAAAAAAAu || size[nb + 1] != 0xAAAAAAAAu || st[0] != 0xAA || st[nb + 1] != 0xAA) {
            printf("batch %u: guard words changed\n", t);
            return 1;
        }
        // (without a status array the sizes are the same)
        std::vector<uint32_t> size2(nb, 0);
        if (lzs_hip_launch_decoded_size_packed(size2.data(), nullptr, d_in, off.data(), len.data(), limit, nb, nullptr)) return 1;
        for (uint32_t b = 0; b < nb; b++)
            if (size2[b] != size[b + 1]) { printf("batch %u: block %u differs without a status array\n", t, b); return 1; }
        for (uint32_t b = 0; b < nb; b++) {
            if (kind[b] == 1) {                                    // (its allocation once more, for the call without lengths)
                buf[b] = (uint8_t *)malloc(keep[b].size() ? keep[b].size() : 1);
                memcpy(buf[b], keep[b].data(), keep[b].size());
            }
            uint32_t s1[3] = {0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu};
            uint8_t t1[3] = {0xAA, 0xAA, 0xAA};
            uint64_t pair[2];
            if (kind[b] == 2) {
                pair[0] = (uint64_t)((uintptr_t)(buf[b] + a0[b]) - base) + 5u;
                pair[1] = pair[0] - 5u;
                free(buf[b]); buf[b] = nullptr;
            } else {
                pair[0] = (uint64_t)((uintptr_t)(buf[b] + a0[b]) - base);
                pair[1] = pair[0] + n[b];
            }
            if (lzs_hip_launch_decoded_size_packed(s1 + 1, t1 + 1, d_in, pair, nullptr, limit, 1, nullptr)) return 1;
            if (s1[0] != 0xAAAAAAAAu || s1[2] != 0xAAAAAAAAu || t1[0] != 0xAA || t1[2] != 0xAA) {
                printf("batch %u, block %u: guard words changed\n", t, b);
                return 1;
            }
            const uint32_t r[4] = {size[b + 1], st[b + 1], s1[1], t1[1]};
            fwrite(r, 4, 4, o);
            free(buf[b]);
            total++;
        }
    }
    fclose(o);
    // without lengths, back to back in one allocation that ends with the last stream's last word: nblocks + 1 offsets are read,
    // wavefront and grid tails, starts at every residue mod 4
    for (uint32_t nb : {1u, 63u, 64u, 65u, 129u}) {
        std::vector<uint64_t> off(nb + 1);
        uint64_t at = 1;
        for (uint32_t b = 0; b < nb; b++) { off[b] = at; at += b % 3u ? 2u + b % 2u : 0u; }
        off[nb] = at;
        uint8_t *in = (uint8_t *)malloc((at + 3) / 4 * 4);
        for (uint64_t i = 0; i < at; i++) in[i] = 0x55;
        for (uint32_t b = 0; b < nb; b++) if (off[b + 1] > off[b]) { in[off[b]] = 0xC0; in[off[b] + 1] = 0x00; }
        std::vector<uint32_t> size(nb + 2u, 7u);
        std::vector<uint8_t> st(nb + 2u, 7u);
        if (lzs_hip_launch_decoded_size_packed(size.data() + 1, st.data() + 1, in, off.data(), nullptr, 100, nb, nullptr)) return 1;
        if (size[0] != 7u || size[nb + 1u] != 7u || st[0] != 7u || st[nb + 1u] != 7u) { printf("dense batch of %u: guard words changed\n", nb); return 1; }
        for (uint32_t b = 0; b < nb; b++)
            if (size[b + 1u] != 0u || st[b + 1u] != (off[b + 1] > off[b] ? 0x04u : 0x03u)) { printf("dense batch of %u: block %u\n", nb, b); return 1; }
        free(in);
    }
    printf("ok %u entries\n", total);
    return 0;
}
