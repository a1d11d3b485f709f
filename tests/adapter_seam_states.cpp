// adapter_seam_states.cpp -- TEST INFRASTRUCTURE, host code only (no GPU library is linked: the adapter's templates that call the
// C ABI are never instantiated here).  What pg_adapter does to a read between the two seams, for tests/test_seam_states_cpu.py:
//   stdin : one read per line  "<sequence as hex, or - for the empty one> <rc_flag>"
//   stdout: per read  "<UnmatchedSeq after apply_rc_flag, hex> <what make_batch(reads, chr_of, rc_flag) uploads for it, hex>"
// (hex, because the sequences hold NUL).  argv[1] = "ref": the read type is tests/ref_shapes.hpp's SPLIT_READ, flipped through its
// own setUnmatchedSeq; "plain": a read type without setUnmatchedSeq, flipped by the adapter's rc_in_place + strip_trailing_non_alnum.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pindel_pg.h"
#include "ref_shapes.hpp"
#include "pg_adapter.hpp"

struct PlainRead {
   std::string UnmatchedSeq;
   char MatchedD;
   unsigned int MatchedRelPos;
   short InsertSize;
};

static int hex_digit(char c)
{
   return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
}

static bool from_hex(const std::string &h, std::string &out)
{
   out.clear();
   if (h == "-") return true;
   if (h.size() & 1) return false;
   for (size_t i = 0; i < h.size(); i += 2) {
      const int a = hex_digit(h[i]), b = hex_digit(h[i + 1]);
      if (a < 0 || b < 0) return false;
      out.push_back((char)(a * 16 + b));
   }
   return true;
}

static std::string to_hex(const unsigned char *p, size_t n)
{
   static const char d[] = "0123456789abcdef";
   if (n == 0) return "-";
   std::string o;
   for (size_t i = 0; i < n; i++) {
      o.push_back(d[p[i] >> 4]);
      o.push_back(d[p[i] & 15]);
   }
   return o;
}

template <class Read>
static int run()
{
   std::vector<Read> reads;
   std::vector<uint8_t> flags;
   std::string line;
   while (std::getline(std::cin, line)) {
      std::istringstream ls(line);
      std::string h, seq;
      int flag = -1;
      ls >> h >> flag;
      if (!from_hex(h, seq) || flag < 0 || flag > 2) {
         std::fprintf(stderr, "bad line %zu\n", reads.size() + 1);
         return 2;
      }
      Read r;
      r.UnmatchedSeq = seq;               // (as it is: the read type's setUnmatchedSeq would already strip the original)
      r.MatchedD = '+';
      r.MatchedRelPos = 1000u + (unsigned)reads.size();
      r.InsertSize = 500;
      reads.push_back(r);
      flags.push_back((uint8_t)flag);
   }
   for (size_t i = 0; i < reads.size(); i++) pg_adapter::apply_rc_flag(reads[i], flags[i]);
   const pg_adapter::Batch b = pg_adapter::make_batch(reads, [](const Read &) { return 0; }, flags.data());
   if (b.off.size() != reads.size() + 1 || b.off.back() != b.seq.size()) {
      std::fprintf(stderr, "make_batch: offsets do not cover the sequence buffer\n");
      return 3;
   }
   for (size_t i = 0; i < reads.size(); i++) {
      const std::string &s = reads[i].UnmatchedSeq;
      if (b.off[i + 1] - b.off[i] != s.size() || b.pos[i] != (int32_t)(1000 + i) || b.strand[i] != '+' || b.isz[i] != 500) {
         std::fprintf(stderr, "make_batch: read %zu\n", i);
         return 3;
      }
      std::cout << to_hex((const unsigned char *)s.data(), s.size()) << ' ' << to_hex(b.seq.data() + b.off[i], s.size()) << '\n';
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc == 2 && !std::strcmp(argv[1], "ref")) return run<SPLIT_READ>();
   if (argc == 2 && !std::strcmp(argv[1], "plain")) return run<PlainRead>();
   std::fprintf(stderr, "usage: %s ref|plain < reads > states\n", argv[0]);
   return 2;
}
