// sv_align_unit.cpp -- the 64-positions-per-step walks of the tandem-duplication and inversion candidates
// (pindel_amd/csrc/pg_sv_align.h, here in their host form) against the host library's one-base-per-iteration loops (left_most_td /
// left_most_inv, pg_host_priv.hpp).  Plain g++, no GPU; also built with -fsanitize=address,undefined:
//   g++ -std=c++17 -Iinclude -Ipindel_amd/csrc -Ipindel_amd/csrc/host tests/sv_align_unit.cpp
// Prints "sv_align_unit ok: <n> checks" and returns 0, or names the first case that differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "pg_host_priv.hpp"
#include "pg_sv_align.h"

namespace {

const unsigned SPACER = 10;                          // (shorter than a step: a step then reads past the string, as it reads guard words on the device)

struct StrRef {                                      // the chromosome string as codes; outside it: a code that equals nothing
    const std::string *s;
    uint32_t operator()(int64_t p) const
    {
        if (p < 0 || p >= (int64_t)s->size()) return PG_SV_OUT;
        switch ((*s)[(size_t)p]) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return PG_VA_N;
        }
    }
};

int n_checks = 0;
const long NO_WANT = 1L << 40;

// want_moved = NO_WANT: not checked.  The walk's length is what BPLeft moved by when no clamp cut it.
bool check_td(const char *what, const std::string &chr, unsigned bl, unsigned br, short bp, long want_moved = NO_WANT)
{
    unsigned a = bl, b = br, c = bl, d = br;
    short p = bp;
    int16_t q = bp;
    const bool e1 = pgh::detail::left_most_td(chr, SPACER, a, b, p);
    const StrRef ref = { &chr };
    const bool e2 = pg_sv_left_most_td(PgVaHostWalk(), ref, (uint32_t)chr.size(), SPACER, c, d, q);
    n_checks++;
    if (a != c || b != d || p != q || e1 != e2 || (want_moved != NO_WANT && (long)(int32_t)(bl - a) != want_moved)) {
        fprintf(stderr, "%s: TD bl %u br %u bp %d: loops give (%u, %u, %d, %d), walks give (%u, %u, %d, %d), wanted a move of %ld\n", what, bl, br, bp,
                a, b, p, (int)e1, c, d, q, (int)e2, want_moved);
        return false;
    }
    return true;
}

bool check_inv(const char *what, const std::string &chr, bool plus, short read_length, unsigned bl, unsigned br, short bp, long want_moved = NO_WANT)
{
    unsigned a = bl, b = br, c = bl, d = br;
    short p = bp;
    int16_t q = bp;
    const bool e1 = pgh::detail::left_most_inv(chr, SPACER, plus, read_length, a, b, p);
    const StrRef ref = { &chr };
    const bool e2 = pg_sv_left_most_inv(PgVaHostWalk(), ref, (uint32_t)chr.size(), SPACER, plus, read_length, c, d, q);
    n_checks++;
    if (a != c || b != d || p != q || e1 != e2 || (want_moved != NO_WANT && (long)(int32_t)(a - bl) != want_moved) || (!e1 && (br - b) != (a - bl))) {
        fprintf(stderr, "%s: INV %c bl %u br %u bp %d: loops give (%u, %u, %d, %d), walks give (%u, %u, %d, %d), wanted a move of %ld\n", what,
                plus ? '+' : '-', bl, br, bp, a, b, p, (int)e1, c, d, q, (int)e2, want_moved);
        return false;
    }
    return true;
}

std::string random_bases(std::mt19937 &g, size_t n, const char *alphabet, size_t k)
{
    std::string s(n, 'A');
    for (char &ch : s) ch = alphabet[g() % k];
    return s;
}

char comp(char c) { return pgh::detail::rc4n(c); }

}  // namespace

int main()
{
    std::mt19937 g(4242);
    const std::string pad(SPACER, 'N');
    bool ok = true;
    char what[96];

    // ---- LeftMostTD: the w bases up to BPLeft repeat before BPRight - 1; BP is large, so nothing is clamped
    for (unsigned w : { 0u, 1u, 63u, 64u, 65u, 130u }) {
        const unsigned D = 300, at = 260;
        std::string bio = random_bases(g, 900, "ACGT", 4);
        for (unsigned t = 0; t < w; t++) bio[at + D - t] = bio[at - t];
        bio[at + D - w] = bio[at - w] == 'A' ? 'C' : 'A';
        snprintf(what, sizeof what, "TD walk of %u", w);
        ok = check_td(what, pad + bio + pad, at, at + D + 1, 200, w) && ok;
        // ... and with a BP the walk reaches or passes: diff >= BP is cut to BP - 1
        for (short bp : { (short)1, (short)2, (short)w, (short)(w + 1) }) {
            if (bp < 1) continue;
            snprintf(what, sizeof what, "TD walk of %u, BP %d", w, bp);
            ok = check_td(what, pad + bio + pad, at, at + D + 1, bp, w == 0 ? 0 : (w >= (unsigned)bp ? bp - 1 : (long)w)) && ok;
        }
    }
    {   // N's on both sides match each other (no N test), and a walk that runs into the spacer ends where the other side is a base
        const unsigned D = 300, at = 260, w = 70;
        std::string bio = random_bases(g, 900, "ACGT", 4);
        for (unsigned t = 0; t < w; t++) bio[at + D - t] = bio[at - t];
        for (unsigned t = 20; t < 30; t++) bio[at + D - t] = bio[at - t] = 'N';
        bio[at + D - w] = bio[at - w] == 'A' ? 'C' : 'A';
        ok = check_td("TD walk over N's on both sides", pad + bio + pad, at, at + D + 1, 200, w) && ok;
        bio[at - 40] = 'N';                           // an N on one side only ends it
        ok = check_td("TD walk ending at an N on one side", pad + bio + pad, at, at + D + 1, 200, 40) && ok;
        std::string bio2 = random_bases(g, 900, "ACGT", 4);
        const unsigned at2 = 99;
        for (unsigned t = 0; t <= at2; t++) bio2[at2 + D - t] = bio2[at2 - t];
        ok = check_td("TD walk reaching the spacer", pad + bio2 + pad, at2, at2 + D + 1, 200, at2 + 1) && ok;
        // the out-of-range branch
        ok = check_td("TD beyond the string", pad + bio2 + pad, 905, 950, 50) && ok;
        ok = check_td("TD right breakpoint beyond the string", pad + bio2 + pad, 300, 915, 50) && ok;
    }
    {   // inside a dinucleotide repeat: a long walk whose two sides overlap
        std::string di = random_bases(g, 200, "AG", 2);
        for (int k = 0; k < 150; k++) di += "CT";
        di += random_bases(g, 200, "AG", 2);
        ok = check_td("TD in a dinucleotide repeat", pad + di + pad, 430, 430 + 41, 140, 140 - 1) && ok;
        ok = check_td("TD in a dinucleotide repeat, odd distance", pad + di + pad, 430, 430 + 40, 140, 0) && ok;
    }

    // ---- LeftMostINV: the w bases from BPLeft + 1 on are the reverse complement of the w bases down from BPRight - 1
    for (unsigned w : { 0u, 1u, 63u, 64u, 65u, 130u }) {
        const unsigned at = 200, D = 500;             // BPLeft, BPRight = at + D
        std::string bio = random_bases(g, 1000, "ACGT", 4);
        for (unsigned t = 0; t < w; t++) bio[at + 1 + t] = comp(bio[at + D - 1 - t]);
        bio[at + 1 + w] = comp(bio[at + D - 1 - w]) == 'A' ? 'C' : 'A';
        for (int plus = 0; plus < 2; plus++) {
            snprintf(what, sizeof what, "INV walk of %u", w);
            // '-': the breakpoints move by the walk (read long enough: no clamp); '+': clamped at most, nothing moves
            ok = check_inv(what, pad + bio + pad, plus != 0, 400, at, at + D, 100, plus ? 0 : (long)w) && ok;
            // the clamps of both anchor strands: '+' diff >= BP, '-' diff + BP >= ReadLength
            for (short rl : { (short)100, (short)101, (short)(100 + w), (short)(101 + w) }) {
                snprintf(what, sizeof what, "INV walk of %u, read length %d", w, rl);
                const long room = (long)rl - 100 - 1;
                ok = check_inv(what, pad + bio + pad, plus != 0, rl, at, at + D, 100, plus || w == 0 ? 0 : ((long)w + 100 >= rl ? room : (long)w)) && ok;
            }
            ok = check_inv("INV walk, BP 1", pad + bio + pad, plus != 0, 400, at, at + D, 1, plus ? 0 : (long)w) && ok;
        }
    }
    {   // a reverse-complement palindrome: the walk passes the middle and goes on outwards until the flanks differ
        const std::string half = random_bases(g, 90, "ACGT", 4);
        std::string pal = half;
        for (size_t k = half.size(); k-- > 0;) pal += comp(half[k]);
        const std::string left = random_bases(g, 300, "ACGT", 4) + "A", right = "A" + random_bases(g, 300, "ACGT", 4);   // A is not T's complement: the walk ends there
        const std::string bio = left + pal + right;
        const unsigned first = (unsigned)left.size();                    // the palindrome's first base (biological index)
        // BPLeft + 1 = its first base, BPRight - 1 = its last: 180 steps match, the 181st compares the two A's
        ok = check_inv("INV walk through a palindrome", pad + bio + pad, false, 400, first - 1, first + 180, 100, 180) && ok;
        ok = check_inv("INV walk through a palindrome, '+' anchor", pad + bio + pad, true, 400, first - 1, first + 180, 100, 0) && ok;
        // starting inside it, off centre by nothing: 60 steps in, through the middle, 30 more each way
        ok = check_inv("INV walk from inside a palindrome", pad + bio + pad, false, 400, first + 29, first + 150, 100, 150) && ok;
        // N's facing each other match (the complement of N is N)
        std::string bio_n = bio;
        bio_n[first + 10] = bio_n[first + 179 - 10] = 'N';
        ok = check_inv("INV walk over N's on both sides", pad + bio_n + pad, false, 400, first - 1, first + 180, 100, 180) && ok;
        bio_n[first + 20] = 'N';
        ok = check_inv("INV walk ending at an N on one side", pad + bio_n + pad, false, 400, first - 1, first + 180, 100, 20) && ok;
        // a whole chromosome that is one palindrome between its spacers would match to the ends of the string; one base short of
        // that the walk ends inside the spacer (N against a base)
        ok = check_inv("INV walk into the spacers", pad + pal + "C" + pad, false, 400, 0u - 1u, 180, 100, 180) && ok;
        // the out-of-range branch
        ok = check_inv("INV beyond the string", pad + bio + pad, false, 400, (unsigned)bio.size() + 5, (unsigned)bio.size() + 50, 100) && ok;
        ok = check_inv("INV at the last base", pad + bio + pad, true, 400, (unsigned)bio.size() - 1, (unsigned)bio.size() + 50, 100) && ok;
    }
    // ---- random strings, low-complexity alphabets included so that walks are not all trivial
    for (int it = 0; it < 4000 && ok; it++) {
        const char *alpha = it % 3 == 0 ? "ACGTN" : (it % 3 == 1 ? "AAAAACN" : "ATAT");
        const size_t k = it % 3 == 0 ? 5 : (it % 3 == 1 ? 7 : 4);
        std::string body = random_bases(g, 60 + g() % 400, alpha, k);
        body[0] = body[body.size() - 1] = 'A';          // (a chromosome that begins with N's could match the spacer all the way out of the string)
        const std::string chr = pad + body + pad;
        const unsigned bio = (unsigned)chr.size() - 2 * SPACER;
        const unsigned bl = 1 + g() % (bio - 4), br = bl + 2 + g() % (bio - bl - 2);
        const short bp = (short)(1 + g() % 150), rl = (short)(bp + 1 + g() % 150);
        ok = check_td("random TD", chr, bl, br, bp) && ok;
        ok = check_inv("random INV", chr, (it & 1) != 0, rl, bl, br, bp) && ok;
    }
    if (!ok) return 1;
    printf("sv_align_unit ok: %d checks\n", n_checks);
    return 0;
}
