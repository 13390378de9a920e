// host_crc_check.cpp -- the scalar drop-in's host CRC (memcached_amd/csrc/
// crc32c_host.cpp) against the oracle at the lengths where its loops change:
// the three-stream merge of crc32c_host_hw runs rounds of 3 x 4096 B and then
// 3 x 256 B behind an 8-B alignment prologue, so every length here sits on, one
// under or just past a round of one of the two sizes, or past the prologue's 0-7
// bytes, from every start 0..8 of a 64-B aligned base.
//
//   gcc -c -fsanitize=address,undefined oracle/crc32c_oracle.c
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -I memcached_amd/csrc
//       host_crc_check.cpp memcached_amd/csrc/crc32c_host.cpp crc32c_oracle.o
//
// Prints "host_crc ok" (and a note when the CPU has no CRC32C instruction, in
// which case crc32c_host_hw is not compared).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "crc32c_host.h"

extern "C" {
uint32_t oracle_crc32c(uint32_t crc, const void *buf, size_t len);
uint32_t oracle_crc32c_bitwise(uint32_t crc, const void *buf, size_t len);
}

namespace {

long g_checked = 0;

#define CHECK_EQ(got, want, ...)                                           \
    do {                                                                   \
        ++g_checked;                                                       \
        const uint32_t g_ = (got), w_ = (want);                            \
        if (g_ != w_) {                                                    \
            fprintf(stderr, "%s:%d: got %08x want %08x: ", __FILE__, __LINE__, g_, w_); \
            fprintf(stderr, __VA_ARGS__);                                  \
            fprintf(stderr, "\n");                                         \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

const size_t kLens[] = {0,     7,     8,     255,   256,   767,   768,   769,   775,   776,
                        1535,  1536,  4095,  4096,  12287, 12288, 12289, 12295, 12296, 13055,
                        13056, 13064, 24575, 24576, 24584, 25351, 36864, 36872, 37640, 65536};
const uint32_t kSeeds[] = {0u, 0xdeadbeefu, 0xffffffffu};
const size_t kSplits[] = {256, 4096};  // the two block sizes of the three-stream loop

typedef uint32_t (*crc_fn)(uint32_t, const void *, size_t);

void compare(const char *name, crc_fn f, const unsigned char *base) {
    for (size_t len : kLens)
        for (size_t off = 0; off <= 8; ++off)
            for (uint32_t seed : kSeeds) {
                const unsigned char *p = base + off;
                const uint32_t want = oracle_crc32c(seed, p, len);
                CHECK_EQ(f(seed, p, len), want, "%s len %zu off %zu seed %08x", name, len, off, seed);
                // the same bytes in two calls, cut at each block size
                for (size_t cut : kSplits)
                    if (len > cut)
                        CHECK_EQ(f(f(seed, p, cut), p + cut, len - cut), want, "%s len %zu off %zu seed %08x cut %zu",
                                 name, len, off, seed, cut);
            }
}

}  // namespace

int main() {
    const size_t kMax = 65536;
    std::vector<unsigned char> store(kMax + 8 + 64);
    unsigned char *base = store.data();
    base += (64 - ((uintptr_t)base & 63u)) & 63u;  // 64-B aligned; starts 0..8 follow
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < kMax + 8; ++i) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        base[i] = (unsigned char)(x >> 32);
    }
    mcrc::host_tables_init();

    // the checker against its own most literal form, on a sample
    for (size_t len : {(size_t)0, (size_t)7, (size_t)769, (size_t)12295, (size_t)37640})
        for (size_t off : {(size_t)0, (size_t)3})
            CHECK_EQ(oracle_crc32c(0xdeadbeefu, base + off, len), oracle_crc32c_bitwise(0xdeadbeefu, base + off, len),
                     "oracle vs bitwise len %zu off %zu", len, off);

    compare("crc32c_host_sw", mcrc::crc32c_host_sw, base);
    if (mcrc::host_has_hw_crc()) compare("crc32c_host_hw", mcrc::crc32c_host_hw, base);
    else printf("note: no CRC32C instruction on this CPU, crc32c_host_hw not compared\n");

    // crc32c_host_combine(crc(a0, A), crc(0, B), |B|) = crc(crc(a0, A), B)
    for (uint64_t len_b : {0ull, 1ull, 4096ull, 40000ull})
        for (uint32_t seed : kSeeds) {
            const uint32_t a = oracle_crc32c(seed, base + 5, 1000);
            const unsigned char *B = base + 1005;
            CHECK_EQ(mcrc::crc32c_host_combine(a, oracle_crc32c(0, B, len_b), len_b), oracle_crc32c(a, B, len_b),
                     "combine len_b %llu seed %08x", (unsigned long long)len_b, seed);
            // a running value of exactly 0 shifts to 0
            CHECK_EQ(mcrc::crc32c_host_combine(0, oracle_crc32c(0, B, len_b), len_b), oracle_crc32c(0, B, len_b),
                     "combine from 0 len_b %llu", (unsigned long long)len_b);
        }
    printf("host_crc ok (%ld comparisons)\n", g_checked);
    return 0;
}
