// indelcol.h -- one column of the bit-vector LCS recurrence (Allison-Dix / Hyyro, 32-bit words of the bit axis per lane) and its
// carry state, for the kernels that run it as a systolic array across the lanes of a wavefront: indel.hip (strings, match masks
// from a table or a compare) and threshwide.hip (series, match words from LDS).  The recurrence and the carry hand-over are
// described in the head of indel.hip.  Include after common.h.
#pragma once
#include <cstdint>

// The carry-ins of the coming column, one bit per lane, and the lanes that never take one.
struct IndelCarry {
    uint64_t first, cin;
    __device__ __forceinline__ void bind(int w) { first = __builtin_amdgcn_ballot_w64(w == 0); }
    __device__ __forceinline__ void reset() { cin = 0; }
};

// One column for the R words of this lane, low word first.  CHECKED: a lane outside its column range keeps V; its carry is
// passed on regardless (the lane above it is out of range in the next step too).
template <int R, bool CHECKED>
__device__ __forceinline__ void indel_column(IndelCarry &cs, uint32_t (&V)[R], const uint32_t (&eq)[R], bool valid)
{
    uint64_t carry = cs.cin;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t u = V[r] & eq[r];
        uint32_t s;
        uint64_t co;
        asm volatile("v_addc_co_u32 %0, %1, %2, %3, %4" : "=v"(s), "=s"(co) : "v"(V[r]), "v"(u), "s"(carry));
        const uint32_t nv = __builtin_amdgcn_bitop3_b32(s, V[r], eq[r], 0xf4);   // s | (V & ~eq)
        V[r] = !CHECKED || valid ? nv : V[r];
        carry = co;
    }
    cs.cin = (carry << 1) & ~cs.first;
}
