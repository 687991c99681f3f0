// playout_cap.h -- playout cap randomization (Wu 2019, "Accelerating Self-Play Learning in Go", section 3.1): which searches of
// the self-play driver are full ones.  A full search is the driver's ordinary search (the driver rule's reads, root noise, a row
// that trains); every other one is a fast search of at most PlayoutCap::fast_reads reads without root noise, whose row is marked
// (replay_row.h: ROW_FLAG_FAST) and only moves the game on.
//
// The decision is a pure function of (seed, absolute game index, ply): never of slot, rank, step or schedule.  Plain C++ for
// g++ and hipcc alike: the host restates it (dbaz_playout_cap_is_full) with the very same code the kernels run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PLAYOUT_HD __host__ __device__
#else
#define PLAYOUT_HD
#endif

struct PlayoutCap {
    uint64_t thresh;    // floor(full_prob * 2^32), 0 .. 2^32
    int32_t fast_reads; // read ceiling of a fast search
    int32_t on;         // 0: every search is a full one
};

#define PLAYOUT_PURPOSE 0x33333333u // counter word 3 of the stream (tree.hip: 0x11111111 fast-forward plies, 0x22222222 move draw)

// Philox4x32-10, output word 0: the ten rounds and constants of philox() in tree.hip, the multiply-high taken from a 64-bit product
PLAYOUT_HD inline uint32_t playout_philox_x(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// counter (lo32(game_idx), hi32(game_idx), ply, PLAYOUT_PURPOSE), key (lo32(seed), hi32(seed)); full when word 0 < thresh
PLAYOUT_HD inline bool playout_is_full(const PlayoutCap &pc, uint64_t seed, int64_t game_idx, uint32_t ply)
{
    if (!pc.on) return true;
    const uint64_t gi = (uint64_t)game_idx;
    const uint32_t x = playout_philox_x((uint32_t)gi, (uint32_t)(gi >> 32), ply, PLAYOUT_PURPOSE, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (uint64_t)x < pc.thresh;
}

// full_prob in [0, 1] (the caller checks) -> the setting; full_prob >= 1 is "off"
inline PlayoutCap playout_cap_make(double full_prob, int32_t fast_reads)
{
    PlayoutCap pc;
    pc.on = full_prob < 1.0 ? 1 : 0;
    pc.thresh = pc.on ? (uint64_t)(full_prob * 4294967296.0) : 4294967296ull;
    pc.fast_reads = pc.on ? fast_reads : 0;
    return pc;
}
