// Stand-alone run of the harness of tests/native/bpsload_host.cpp for the host sanitizers (a program of its own: nothing is
// preloaded).  The reads of the test suite's length list, padding bits set, go through every chunking and are compared with
// a serial unpack; every array is an exact-size heap allocation, so a read or write past an end is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" int64_t bl_host_unpack(const uint8_t *bps, const int64_t *boff, const int32_t *rlen, int64_t n, const int64_t *chunk_first,
                                  int64_t nchunks, uint8_t *out, int64_t out_len);

static uint32_t rnd(uint32_t &s)
{
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

static int run(const std::vector<int32_t> &rlen, uint32_t seed, const char *name)
{
    const int64_t n = (int64_t)rlen.size();
    std::vector<int64_t> boff((size_t)n);
    std::vector<uint8_t> bps, want;
    for (int64_t r = 0; r < n; r++) {
        boff[(size_t)r] = (int64_t)bps.size();
        const int32_t l = rlen[(size_t)r];
        bps.resize(bps.size() + (size_t)((l + 3) / 4), 0);
        for (int32_t x = 0; x < l; x++) {
            const uint8_t code = (uint8_t)(rnd(seed) & 3);
            want.push_back(code);
            bps[(size_t)boff[(size_t)r] + (size_t)(x >> 2)] |= (uint8_t)(code << (6 - 2 * (x & 3)));
        }
        if (l & 3) bps.back() |= (uint8_t)((1u << (8 - 2 * (l & 3))) - 1);  // the padding bits, set
    }
    const int64_t total = (int64_t)want.size();
    std::vector<std::vector<int64_t>> chunkings;
    chunkings.push_back({0, n});
    std::vector<int64_t> single;
    for (int64_t r = 0; r <= n; r++) single.push_back(r);
    chunkings.push_back(single);
    int64_t acc = 0;
    for (int64_t r = 0; r < n; r++) {  // a chunk that ends exactly on a 16-byte window
        acc += rlen[(size_t)r];
        if (r + 1 < n && acc % 16 == 0 && acc > 0) {
            chunkings.push_back({0, r + 1, n});
            break;
        }
    }
    chunkings.push_back({0, n / 3, n / 3, 2 * n / 3, n});  // with an empty chunk
    int bad = 0;
    for (const std::vector<int64_t> &cf : chunkings) {
        void *mem = nullptr;  // 16-byte aligned and exactly `total` bytes long
        if (posix_memalign(&mem, 16, (size_t)total) != 0) return 1;
        uint8_t *out = (uint8_t *)mem;
        memset(out, 0xAA, (size_t)total);
        const int64_t st = bl_host_unpack(bps.data(), boff.data(), rlen.data(), n, cf.data(), (int64_t)cf.size() - 1, out, total);
        bool ok = st >= 0 && memcmp(out, want.data(), (size_t)total) == 0;
        if (!ok) {
            fprintf(stderr, "%s: %zu chunk(s): the lanes' bytes differ (returned %lld)\n", name, cf.size() - 1, (long long)st);
            bad++;
        }
        free(out);
    }
    return bad;
}

int main()
{
    std::vector<int32_t> lens = {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 1000};
    int bad = 0, nrun = 0;
    uint32_t seed = 7;
    for (int rep = 0; rep < 40; rep++) {
        std::vector<int32_t> order = lens;
        for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rnd(seed) % i]);
        if (rep & 1) order.insert(order.begin() + (long)(rnd(seed) % order.size()), 0);  // a read without a base
        bad += run(order, seed + 100, ("order " + std::to_string(rep)).c_str());
        nrun++;
    }
    bad += run({1}, 3, "one base");
    bad += run({16}, 4, "one window");
    bad += run({4000}, 5, "one read");
    nrun += 3;
    printf("%d run(s), %d failed\n", nrun, bad);
    return bad ? 1 : 0;
}
