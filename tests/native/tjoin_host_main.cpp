// Stand-alone driver of tests/native/tjoin_host.cpp for a build under the host sanitizers (a program of its own: nothing
// is preloaded): the shapes of tests/test_tjoin_host.py.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

extern "C" int64_t tjoin_host_check(int32_t n, int32_t ndistinct, int32_t kbits, int32_t clash, int32_t tcap, int32_t strands,
                                    uint64_t seed);

int main()
{
    int64_t bad = 0;
    const int32_t ns[] = {0, 1, 100, 2500, 8191, 8192};
    for (int32_t n : ns)
        for (int32_t nd : {1, 7, 300, 8192})
            for (int32_t clash = 0; clash < 2; clash++) {
                if (clash && nd > 300) continue;
                const int64_t b = tjoin_host_check(n, nd, clash ? 32 : 28, clash, 4, 3, (uint64_t)(n * 31 + nd));
                if (b) printf("n %d distinct %d clash %d: %lld disagreements\n", n, nd, clash, (long long)b);
                bad += b;
            }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
