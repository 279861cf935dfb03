// Drives pool_layout (annchor_amd/csrc/poollayout.h) from stdin for tests/test_pool_layout_host.py.
// A case: "nx min_len max_len align cap" and then nx lengths.  Its answer, one line: "ok total maxlen off_0 .. off_{nx-1}", or
// "refused KIND at" with KIND one of short, long, large.
#include <cstdio>
#include <vector>

#include "poollayout.h"

int main()
{
    long long nx, cap;
    int min_len, max_len, align;
    while (scanf("%lld %d %d %d %lld", &nx, &min_len, &max_len, &align, &cap) == 5) {
        std::vector<int32_t> lens((size_t)nx);
        for (auto &l : lens)
            if (scanf("%d", &l) != 1) return 2;
        const PoolLayout L = pool_layout(lens.data(), nx, min_len, max_len, (size_t)align, (size_t)cap);
        if (L.refusal != PoolRefusal::None) {
            printf("refused %s %lld\n", L.refusal == PoolRefusal::TooShort ? "short" : L.refusal == PoolRefusal::TooLong ? "long" : "large",
                   (long long)L.at);
            continue;
        }
        printf("ok %zu %d", L.total, L.maxlen);
        for (int32_t o : L.offs) printf(" %d", o);
        printf("\n");
    }
    return 0;
}
