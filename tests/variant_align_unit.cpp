// variant_align_unit.cpp -- the 64-positions-per-step alignment walks the device classifier uses (pindel_amd/csrc/pg_variant_align.h,
// here in their host form) against the host library's one-base-per-iteration loops (real_start_deletion / real_start_insertion,
// pg_host_priv.hpp).  Plain g++, no GPU:  g++ -std=c++17 -Iinclude -Ipindel_amd/csrc -Ipindel_amd/csrc/host tests/variant_align_unit.cpp
// Prints "variant_align_unit ok: <n> checks" and returns 0, or names the first case that differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "pg_host_priv.hpp"
#include "pg_variant_align.h"

namespace {

const unsigned SPACER = 10;                          // (shorter than a step: a step then reads past the string, as it reads guard words on the device)

struct StrRef {                                      // the chromosome string as codes; outside it: N, like the guard words
    const std::string *s;
    uint32_t operator()(int64_t p) const
    {
        if (p < 0 || p >= (int64_t)s->size()) return PG_VA_N;
        switch ((*s)[(size_t)p]) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return PG_VA_N;
        }
    }
};
struct StrIns {                                      // the inserted string before any rotation; a byte outside ACGTN equals nothing
    const std::string *s;
    uint32_t operator()(uint32_t j) const
    {
        switch ((*s)[j]) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        case 'N': return PG_VA_N;
        default: return PG_VA_NONE;
        }
    }
};

int n_checks = 0;

bool check_deletion(const char *what, const std::string &chr, unsigned rs, unsigned re, long want_left = -1)
{
    unsigned a = rs, b = re, c = rs, d = re;
    pgh::detail::real_start_deletion(chr, SPACER, a, b);
    const StrRef ref = { &chr };
    pg_va_real_start_deletion(PgVaHostWalk(), ref, SPACER, c, d);
    n_checks++;
    if (a != c || b != d || (want_left >= 0 && (long)(rs - a) != want_left)) {
        fprintf(stderr, "%s: deletion rs %u re %u: loops give (%u, %u), walks give (%u, %u), left walk wanted %ld\n", what, rs, re, a, b, c, d, want_left);
        return false;
    }
    return true;
}

bool check_insertion(const char *what, const std::string &chr, const std::string &ins, unsigned rs, unsigned re, long want_rot = 1 << 30)
{
    unsigned a = rs, b = re, c = rs, d = re;
    std::string rotated = ins;
    pgh::detail::real_start_insertion(chr, SPACER, rotated, a, b);
    const StrRef ref = { &chr };
    const StrIns code = { &ins };
    const int32_t rot = pg_va_real_start_insertion(PgVaHostWalk(), ref, code, (uint32_t)ins.size(), SPACER, c, d);
    const long len = (long)ins.size(), r = ((rot % len) + len) % len;
    const std::string mine = ins.substr((size_t)r) + ins.substr(0, (size_t)r);
    n_checks++;
    if (a != c || b != d || mine != rotated || (want_rot != (1 << 30) && want_rot != rot)) {
        fprintf(stderr, "%s: insertion '%s' rs %u re %u: loops give (%u, %u, '%s'), walks give (%u, %u, '%s', rotation %d)\n", what, ins.c_str(),
                rs, re, a, b, rotated.c_str(), c, d, mine.c_str(), rot);
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

}  // namespace

int main()
{
    std::mt19937 g(12345);
    const std::string pad(SPACER, 'N');
    bool ok = true;

    // a deletion of D bases whose left walk is exactly w long: the w bases up to the left breakpoint repeat before the right one
    for (unsigned w : { 0u, 1u, 63u, 64u, 65u, 127u, 128u, 200u }) {
        const unsigned D = 300, at = 260;             // biological index of the left breakpoint's base
        std::string bio = random_bases(g, 900, "ACGT", 4);
        for (unsigned t = 0; t < w; t++) bio[at + D - t] = bio[at - t];
        bio[at + D - w] = bio[at - w] == 'A' ? 'C' : 'A';
        const std::string chr = pad + bio + pad;
        char what[64];
        snprintf(what, sizeof what, "left walk of %u", w);
        ok = check_deletion(what, chr, at, at + D + 1, w) && ok;
    }
    {   // ... that ends on an N (equal characters, but N), and one that reaches the spacer
        const unsigned D = 300, at = 260, w = 70;
        std::string bio = random_bases(g, 900, "ACGT", 4);
        for (unsigned t = 0; t < w; t++) bio[at + D - t] = bio[at - t];
        bio[at - w] = bio[at + D - w] = 'N';
        ok = check_deletion("left walk ending on N", pad + bio + pad, at, at + D + 1, w) && ok;
        std::string bio2 = random_bases(g, 900, "ACGT", 4);
        const unsigned at2 = 99;                      // 100 bases from the chromosome's first to the breakpoint: all of them repeat
        for (unsigned t = 0; t <= at2; t++) bio2[at2 + D - t] = bio2[at2 - t];
        ok = check_deletion("left walk reaching the spacer", pad + bio2 + pad, at2, at2 + D + 1, at2 + 1) && ok;
    }
    {   // inside a 300-base homopolymer and a dinucleotide repeat: both walks are long and the two copies overlap
        std::string bio = random_bases(g, 200, "CGT", 3) + std::string(300, 'A') + random_bases(g, 200, "CGT", 3);
        ok = check_deletion("homopolymer", pad + bio + pad, 350, 350 + 21) && ok;
        std::string di = random_bases(g, 200, "AG", 2);
        for (int k = 0; k < 150; k++) di += "CT";
        di += random_bases(g, 200, "AG", 2);
        ok = check_deletion("dinucleotide repeat", pad + di + pad, 330, 330 + 41) && ok;
        ok = check_deletion("dinucleotide repeat, odd size", pad + di + pad, 330, 330 + 40) && ok;
    }
    {   // insertions: one base in a homopolymer (every rotation is the same string), a whole repeat unit (the rotation wraps)
        std::string bio = random_bases(g, 100, "CGT", 3) + std::string(150, 'A') + random_bases(g, 100, "CGT", 3);
        ok = check_insertion("one base in a homopolymer", pad + bio + pad, "A", 170, 171) && ok;
        std::string rep = random_bases(g, 100, "AT", 2);
        for (int k = 0; k < 40; k++) rep += "ACG";
        rep += random_bases(g, 100, "AT", 2);
        // between two units: the string walks right to the end of the repeat and back to its start
        ok = check_insertion("unit ACG between units", pad + rep + pad, "ACG", 100 + 3 * 20 - 1, 100 + 3 * 20) && ok;
        ok = check_insertion("unit CGA inside a unit", pad + rep + pad, "CGA", 100 + 3 * 20, 100 + 3 * 20 + 1) && ok;
        ok = check_insertion("unit GAC inside a unit", pad + rep + pad, "GAC", 100 + 3 * 20 + 1, 100 + 3 * 20 + 2) && ok;
        ok = check_insertion("two units", pad + rep + pad, "ACGACG", 100 + 3 * 30 - 1, 100 + 3 * 30) && ok;
        ok = check_insertion("no match at all", pad + rep + pad, "TTT", 100 + 3 * 20 - 1, 100 + 3 * 20, 0) && ok;
        ok = check_insertion("a string with an N and a NUL", pad + rep + pad, std::string("AN\0G", 4), 100 + 3 * 20 - 1, 100 + 3 * 20) && ok;
        // right of the repeat's start only: the net rotation is negative (the second loop passes where the first began)
        ok = check_insertion("left of the insertion point only", pad + rep + pad, "ACG", 100 + 3 * 40 - 1, 100 + 3 * 40) && ok;
    }
    // random ACGTN strings, low-complexity alphabets included so that walks are not all trivial
    for (int it = 0; it < 4000 && ok; it++) {
        const char *alpha = it % 3 == 0 ? "ACGTN" : (it % 3 == 1 ? "AAAAACN" : "ACAC");
        const size_t k = it % 3 == 0 ? 5 : (it % 3 == 1 ? 7 : 4);
        const std::string chr = pad + random_bases(g, 50 + g() % 400, alpha, k) + pad;
        const unsigned bio = (unsigned)chr.size() - 2 * SPACER;
        const unsigned rs = g() % (bio - 2), re = rs + 2 + g() % (bio - rs - 1);
        ok = check_deletion("random deletion", chr, rs, re > bio ? bio : re) && ok;
        const unsigned is = g() % (bio - 1);
        ok = check_insertion("random insertion", chr, random_bases(g, 1 + g() % 6, alpha, k), is, is + 1) && ok;
    }
    if (!ok) return 1;
    printf("variant_align_unit ok: %d checks\n", n_checks);
    return 0;
}
