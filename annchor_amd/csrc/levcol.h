// levcol.h -- one column of the bit-parallel Levenshtein recurrence (Myers / Hyyro, one 32-bit word of the pattern per
// lane) for the kernels of lev.hip that keep their match masks in LDS: k_lev_f, k_lev_p2, k_lev_a2, k_lev_ap.
// Only the column and its carry state live here.  What surrounds it -- staging, the match-mask build, the rows mask, the
// fused pick, and the step bounds, column walk and F / B' join of the forward / backward kernels -- is levhalf.h; the
// kernels, their argument blocks and launchers are lev.hip.
//
// A lane holds the vertical deltas of its word (vp / vn, disjoint by induction) and gets the horizontal deltas of the
// row above its word from the lane below it in lane order: the top bits of that lane's hp / hn in the previous column
// (the wave is a systolic array: lane w works on column k - w).  The first lane of a pair slot sees the row above the
// pattern instead: D[0][j] - D[0][j-1] = +1, i.e. hp carry 1, hn carry 0.
//
//   c   = hn carry-in (0 / 1)
//   xv  = eq | c | vn                      the X term with vn folded in (vn & vp == 0, so (c | eq) & vp is unchanged)
//   d0  = ((((c | eq) & vp) + vp) ^ vp) | xv
//   hp  = vn | ~(d0 | vp),  hn = d0 & vp
//   hps = (hp << 1) | hp carry-in,  hns = (hn << 1) | hn carry-in
//   vp' = hns | ~(d0 | hps),  vn' = hps & d0
//
// Two ways to move the carries between lanes:
//   LEV_CARRY_DPP   hp / hn travel as words through `wave_shr:1` DPP moves whose second operand is a per-lane constant that
//                   also plants the first lane's carries (v_or_b32_dpp / v_and_b32_dpp), issued as soon as hp / hn of a column
//                   exist, for the NEXT column; c is a v_lshrrev, the shifts a v_alignbit and a v_lshl_or (or a second
//                   v_alignbit): 13 VALU per column.
//   LEV_CARRY_MASK  the carries of all 64 lanes are two wave-wide lane masks in SGPR pairs.  (hp << 1) | carry is
//                   hp + hp + carry: one v_addc_co_u32 yields the shifted word AND, as its carry-out mask, hp's top bit of
//                   every lane -- what the next lane needs in the next column.  The masks move up one lane and take the
//                   first lanes' constants on the scalar unit (s_lshl_b64, s_or_b64 / s_andn2_b64: register-only scalar
//                   ALU), c is a v_cndmask_b32 on the hn mask: 11 VALU + 4 SALU per column.
//                   The carry-out is taken from EVERY lane in every column, so the column loop must run with all 64 lanes
//                   enabled (a disabled lane's carry-out reads 0).
// (The kernels add one v_lshl_add_u32 per column for the address of the next match-mask row.)
#pragma once
#include <cstdint>

enum { LEV_CARRY_DPP = 0, LEV_CARRY_MASK = 1 };

__device__ __forceinline__ uint32_t dpp_shr1_or(uint32_t v, uint32_t m)
{
    // lane l: v[l-1] | m[l]; lane 0 (no source lane, bound_ctrl): 0 | m[0]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true) | m;
}
__device__ __forceinline__ uint32_t dpp_shr1_and(uint32_t v, uint32_t m)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true) & m;
}

template <int CARRY> struct LevCarry;

template <> struct LevCarry<LEV_CARRY_DPP> {
    uint32_t hp_or, hn_and;     // carry-in constants of this lane
    uint32_t up_hp;             // hp carry-in of the coming column: the top bit of this word
    uint32_t c;                 // hn carry-in of the coming column, 0 / 1
    // w: index of this lane's word inside its pair slot
    __device__ __forceinline__ void bind(int w)
    {
        hp_or = w == 0 ? 0x80000000u : 0u;
        hn_and = w == 0 ? 0u : 0xffffffffu;
        asm volatile("" : "+v"(hp_or), "+v"(hn_and));   // opaque: keeps them operands of v_or_b32_dpp / v_and_b32_dpp (not a select)
    }
    __device__ __forceinline__ void reset() { up_hp = hp_or; c = 0; }   // before the first column of a pair: hp = hn = 0 above
};

template <> struct LevCarry<LEV_CARRY_MASK> {
    uint64_t first;             // lanes that are the first of a pair slot
    uint64_t hp_in, hn_in;      // carry-ins of the coming column, one bit per lane
    uint32_t c;                 // this lane's bit of hn_in as 0 / 1
    __device__ __forceinline__ void bind(int w) { first = __builtin_amdgcn_ballot_w64(w == 0); }
    __device__ __forceinline__ void reset() { hp_in = first; hn_in = 0; c = 0; }
};

// One column: vp / vn of this lane's word advance by the text symbol whose match mask is `eq`.  CHECKED: a lane outside its
// column range (`valid` false) keeps vp / vn; its carries are passed on regardless (nobody in range reads them).
// `fetch` issues the caller's LDS reads for the columns ahead (the kernels keep one to three columns in flight).
//
// The order of a column's instructions is pinned (a scheduling barrier after every statement): an instruction that reads the
// result of the one just before it issues later than an independent one, so the chain t -> sm -> d0 -> hn -> hns -> vp' is
// interleaved with everything that is not on it -- xv, the LDS reads, hp, hps, vn' and the carry hand-over, which prepares
// the NEXT column's carry-ins as soon as hp / hn exist.  Measured on isolated launches against the compiler's own order:
// k_lev_f (masks) 225 -> 215 us per 62 000 pairs, k_lev_a2 (DPP) 26.8 -> 24.6 us per round.
#define LEV_PIN() __builtin_amdgcn_sched_barrier(0)
template <int CARRY, bool CHECKED, class Fetch>
__device__ __forceinline__ void lev_column(LevCarry<CARRY> &cs, uint32_t &vp, uint32_t &vn, uint32_t eq, bool valid, Fetch fetch)
{
    if constexpr (CARRY == LEV_CARRY_DPP) {
        const uint32_t c = cs.c;
        LEV_PIN();
        const uint32_t t = __builtin_amdgcn_bitop3_b32(c, eq, vp, 0xa8);        // (c | eq) & vp
        LEV_PIN();
        const uint32_t xv = __builtin_amdgcn_bitop3_b32(eq, c, vn, 0xfe);       // eq | c | vn
        LEV_PIN();
        const uint32_t sm = t + vp;
        LEV_PIN();
        fetch();
        LEV_PIN();
        const uint32_t d0 = __builtin_amdgcn_bitop3_b32(sm, vp, xv, 0xbe);      // (sm ^ vp) | xv
        LEV_PIN();
        const uint32_t hn = d0 & vp;
        LEV_PIN();
        const uint32_t hp = __builtin_amdgcn_bitop3_b32(vn, d0, vp, 0xf1);      // vn | ~(d0 | vp)
        LEV_PIN();
        const uint32_t hns = (hn << 1) | c;                                     // v_lshl_or_b32
        LEV_PIN();
        const uint32_t hps = __builtin_amdgcn_alignbit(hp, cs.up_hp, 31);       // (hp << 1) | carry from the word above
        LEV_PIN();
        const uint32_t up_hn = dpp_shr1_and(hn, cs.hn_and);
        LEV_PIN();
        const uint32_t nvp = __builtin_amdgcn_bitop3_b32(hns, d0, hps, 0xf1);   // hns | ~(d0 | hps)
        LEV_PIN();
        cs.up_hp = dpp_shr1_or(hp, cs.hp_or);
        LEV_PIN();
        const uint32_t nvn = hps & d0;
        LEV_PIN();
        cs.c = up_hn >> 31;
        vp = !CHECKED || valid ? nvp : vp;
        vn = !CHECKED || valid ? nvn : vn;
        LEV_PIN();
    } else {
        const uint32_t c = cs.c;
        uint32_t hps, hns, cn;
        uint64_t cop, con;
        LEV_PIN();
        const uint32_t t = __builtin_amdgcn_bitop3_b32(c, eq, vp, 0xa8);        // (c | eq) & vp
        LEV_PIN();
        const uint32_t xv = __builtin_amdgcn_bitop3_b32(eq, c, vn, 0xfe);       // eq | c | vn
        LEV_PIN();
        const uint32_t sm = t + vp;
        LEV_PIN();
        fetch();
        LEV_PIN();
        const uint32_t d0 = __builtin_amdgcn_bitop3_b32(sm, vp, xv, 0xbe);      // (sm ^ vp) | xv
        LEV_PIN();
        const uint32_t hn = d0 & vp;
        LEV_PIN();
        const uint32_t hp = __builtin_amdgcn_bitop3_b32(vn, d0, vp, 0xf1);      // vn | ~(d0 | vp)
        LEV_PIN();
        asm volatile("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(hns), "=s"(con) : "v"(hn), "s"(cs.hn_in));
        LEV_PIN();
        asm volatile("v_addc_co_u32 %0, %1, %2, %2, %3" : "=v"(hps), "=s"(cop) : "v"(hp), "s"(cs.hp_in));
        LEV_PIN();
        cs.hn_in = (con << 1) & ~cs.first;
        LEV_PIN();
        const uint32_t nvp = __builtin_amdgcn_bitop3_b32(hns, d0, hps, 0xf1);   // hns | ~(d0 | hps)
        LEV_PIN();
        cs.hp_in = (cop << 1) | cs.first;
        LEV_PIN();
        const uint32_t nvn = hps & d0;
        LEV_PIN();
        asm volatile("v_cndmask_b32 %0, 0, 1, %1" : "=v"(cn) : "s"(cs.hn_in));
        cs.c = cn;
        vp = !CHECKED || valid ? nvp : vp;
        vn = !CHECKED || valid ? nvn : vn;
        LEV_PIN();
    }
}
#undef LEV_PIN
