// poollayout.h -- where the members of a ragged pool start.  Plain C++17: no HIP, no context, no message texts, so that a host
// program can test it on its own (tests/pool_layout_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

enum class PoolRefusal { None, TooShort, TooLong, TooLarge };

// offs[s]: the start of member s, in elements: the members' lengths before it, each rounded up to `align`.  A refusal names the
// first member that caused it (`at`); offs, total and maxlen are then unspecified.
struct PoolLayout {
    std::vector<int32_t> offs;
    size_t total = 0;   // elements, padding included
    int maxlen = 0;
    PoolRefusal refusal = PoolRefusal::None;
    int64_t at = -1;
};

// min_len: 0 or 1 (TooShort below it, a negative length included); max_len: TooLong above it; align: 1, 8 or 16 elements;
// cap <= 2^31: the running total stays BELOW it (TooLarge at the member that reaches it), so every start fits an int32.
inline PoolLayout pool_layout(const int32_t *lens, int64_t nx, int min_len, int max_len, size_t align, size_t cap)
{
    PoolLayout L;
    L.offs.resize((size_t)nx);
    int32_t *const offs = L.offs.data();
    size_t total = 0;
    int maxlen = 0;
    for (int64_t s = 0; s < nx; ++s) {
        const int32_t len = lens[s];
        if (len < min_len || len > max_len) {
            L.refusal = len < min_len ? PoolRefusal::TooShort : PoolRefusal::TooLong;
            L.at = s;
            break;
        }
        offs[s] = (int32_t)total;
        total += ((size_t)len + align - 1) & ~(align - 1);
        if (len > maxlen) maxlen = len;
        if (total >= cap) {
            L.refusal = PoolRefusal::TooLarge;
            L.at = s;
            break;
        }
    }
    L.total = total;
    L.maxlen = maxlen;
    return L;
}
