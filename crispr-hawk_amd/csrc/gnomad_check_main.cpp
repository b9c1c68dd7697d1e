// gnomad_check_main.cpp - a stand-alone run of the host side of the gnomAD converter (hawk_host_gnomad_lines and
// hawk_host_f32_repr, hawk_hostutil.hip; the rules: hawk_gnomad.h) for a sanitizer build: `make asan-gnomad` compiles this file
// and hawk_hostutil.hip with -fsanitize=address,undefined and runs the program.  The seam panel of the device tests - the key
// at every offset around a 4096-byte sweep, its value across it, records of 4095 .. 70001 bytes, the shortest record, the key
// first and last with every line end - each in a text buffer of EXACTLY its size and into a blob of EXACTLY the size the length
// pass named (a byte read or written beyond either is a heap overflow the sanitizer sees); then every value and flag case
// against the flags they must give, the refused arguments with the outputs untouched, and the float texts.  Then the long fields:
// every field starting at 4095 / 4096 / 4097, an ALT of 5000 alleles and one of 100 000 bytes, field offsets, spans and lines
// held to a naive splitter written here.  Not part of the library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hawk.h"

namespace {
const char* POPS[10] = {"afr", "ami", "amr", "asj", "eas", "fin", "nfe", "mid", "sas", "remaining"};
int failures = 0;
void fail(const std::string& what) { printf("FAILED: %s\n", what.c_str()); ++failures; }

struct Keys {
  std::vector<uint8_t> blob;
  std::vector<uint64_t> off{0};
  void add(const std::string& k) { blob.insert(blob.end(), k.begin(), k.end()); off.push_back(blob.size()); }
};
Keys pop_keys() {
  Keys k;
  for (const char* p : POPS) k.add(std::string("AC_") + p);
  return k;
}
std::string record(const std::string& afr, const std::string& rest, const std::string& front = "", const std::string& back = "",
                   const std::string& filter = "PASS", const std::string& alt = "G", const std::string& pos = "100", const std::string& af = "AF=0.5") {
  std::string s = "chr21\t" + pos + "\t.\tA\t" + alt + "\t.\t" + filter + "\t" + front;
  if (!afr.empty()) s += afr + ";";
  for (int i = 1; i < 10; ++i) s += std::string("AC_") + POPS[i] + "=" + rest + ";";
  s += af + back;
  return s;
}
struct Result {
  int rc = 0;
  std::vector<uint32_t> mask, fo, qs, as;
  std::vector<uint8_t> flags, blob;
  std::vector<uint64_t> off;
  uint64_t n_bytes = 0, n_kept = 0;
};
// the records of `lines` (ended as `ends` says) through scan, pool and lines; QUAL "." and AF texts from hawk_host_f32_repr
Result run(const std::vector<std::string>& lines, const std::vector<std::string>& ends, const Keys& K, int keep) {
  std::vector<uint8_t> text;  // exactly the bytes: no slack behind the last '\n'
  std::vector<uint64_t> lo{0};
  for (size_t i = 0; i < lines.size(); ++i) {
    text.insert(text.end(), lines[i].begin(), lines[i].end());
    const std::string& e = ends.empty() ? std::string("\n") : ends[i];
    text.insert(text.end(), e.begin(), e.end());
    lo.push_back(text.size());
  }
  const uint64_t n = lines.size();
  Result R;
  R.mask.assign(n, 77); R.flags.assign(n, 77); R.fo.assign(n * 8, 77); R.qs.assign(n * 2, 77); R.as.assign(n * 2, 77); R.off.assign(n + 1, 77);
  R.rc = hawk_host_gnomad_lines(text.data(), text.size(), lo.data(), n, K.blob.data(), K.off.data(), (uint32_t)K.off.size() - 1, keep, R.mask.data(),
                                R.flags.data(), R.fo.data(), R.qs.data(), R.as.data(), nullptr, nullptr, nullptr, 0, nullptr, &R.n_bytes, &R.n_kept);
  if (R.rc != HAWK_OK) return R;
  std::vector<uint64_t> start;
  std::vector<uint32_t> len;
  for (int pass = 0; pass < 2; ++pass)
    for (uint64_t i = 0; i < n; ++i) {
      if (R.flags[i]) continue;
      const uint32_t* sp = pass == 0 ? &R.qs[i * 2] : &R.as[i * 2];
      start.push_back(sp[1] == 0xffffffffu ? 0 : lo[i] + sp[0]);
      len.push_back(sp[1]);
    }
  const uint64_t ns = start.size();
  std::vector<uint64_t> poff(ns + 1, 0);
  std::vector<uint8_t> st(ns + 1, 0), pool;
  // QUAL prints "." for ".", AF prints None: two calls, one per half of the pool
  std::vector<uint64_t> o1(ns / 2 + 1), o2(ns / 2 + 1);
  int rc = hawk_host_f32_repr(text.data(), start.data(), len.data(), ns / 2, ".", nullptr, 0, o1.data(), st.data(), 2);
  if (rc != HAWK_OK && rc != HAWK_E_CAPACITY) { fail("f32 length pass"); R.rc = rc; return R; }
  std::vector<uint8_t> b1(o1[ns / 2]), b2;
  if (hawk_host_f32_repr(text.data(), start.data(), len.data(), ns / 2, ".", b1.data(), b1.size(), o1.data(), st.data(), 2) != HAWK_OK) fail("f32 fill pass");
  rc = hawk_host_f32_repr(text.data(), start.data() + ns / 2, len.data() + ns / 2, ns / 2, "None", nullptr, 0, o2.data(), st.data() + ns / 2, 1);
  if (rc != HAWK_OK && rc != HAWK_E_CAPACITY) { fail("f32 length pass (AF)"); R.rc = rc; return R; }
  b2.resize(o2[ns / 2]);
  if (hawk_host_f32_repr(text.data(), start.data() + ns / 2, len.data() + ns / 2, ns / 2, "None", b2.data(), b2.size(), o2.data(), st.data() + ns / 2, 1) != HAWK_OK)
    fail("f32 fill pass (AF)");
  pool = b1;
  pool.insert(pool.end(), b2.begin(), b2.end());
  for (uint64_t j = 0; j <= ns / 2; ++j) { poff[j] = o1[j]; poff[ns / 2 + j] = o1[ns / 2] + o2[j]; }
  rc = hawk_host_gnomad_lines(text.data(), text.size(), lo.data(), n, K.blob.data(), K.off.data(), (uint32_t)K.off.size() - 1, keep, nullptr, nullptr,
                              nullptr, nullptr, nullptr, pool.data(), poff.data(), nullptr, 0, R.off.data(), &R.n_bytes, &R.n_kept);
  if (rc != (R.n_bytes ? HAWK_E_CAPACITY : HAWK_OK)) { fail("lines: length pass"); R.rc = rc; return R; }
  R.blob.assign(R.n_bytes, 0);
  R.rc = hawk_host_gnomad_lines(text.data(), text.size(), lo.data(), n, K.blob.data(), K.off.data(), (uint32_t)K.off.size() - 1, keep, nullptr, nullptr,
                                nullptr, nullptr, nullptr, pool.data(), poff.data(), R.blob.data(), R.blob.size(), R.off.data(), &R.n_bytes, &R.n_kept);
  return R;
}
std::string line_of(const Result& R, uint64_t i) { return std::string(R.blob.begin() + R.off[i], R.blob.begin() + R.off[i + 1]); }
std::string gts(uint32_t mask) {
  std::string s;
  for (int k = 0; k < 10; ++k) s += (mask >> k) & 1 ? "\t0/1" : "\t0/0";
  return s + "\n";
}
// ---- the naive splitter the long-field cases are held to
std::vector<std::string> split(const std::string& s, char d) {
  std::vector<std::string> out(1);
  for (char c : s) {
    if (c == d) out.emplace_back();
    else out.back().push_back(c);
  }
  return out;
}
std::string rep(const std::string& unit, size_t n) {
  std::string s;
  while (s.size() < n) s += unit;
  return s.substr(0, n);
}
std::string alt_of_len(size_t n) { return n & 1 ? "G" + rep(",T", n - 1) : "GA" + rep(",T", n - 2); }
std::string filter_of_len(size_t n) { return (n - 4) & 1 ? "PASS;qq" + rep(";q", n - 7) : "PASS" + rep(";q", n - 4); }
// a record of eight fields whose field f starts at byte o: the field in front of it lengthened (ALT in front of FILTER: QUAL stays short)
std::string long_record(int f, size_t o, bool* has_af) {
  std::vector<std::string> fl = {"1", "1", ".", "A", "G", ".", "PASS"};
  const int how = f - 1 == 5 ? 4 : f - 1;
  size_t start = 0, between = 0;
  for (int k = 0; k < how; ++k) start += fl[k].size() + 1;
  for (int k = how + 1; k < f; ++k) between += fl[k].size() + 1;
  const size_t n = o - start - 1 - between;
  fl[how] = how == 0 ? rep("chrX", n) : how == 1 ? rep("1234567890", n) : how == 2 ? rep("rs77", n) : how == 3 ? rep("ACGT", n) : how == 4 ? alt_of_len(n) : filter_of_len(n);
  *has_af = how != 4;
  std::string s;
  for (const std::string& x : fl) s += x + "\t";
  s += "AC_afr=0";
  for (int i = 1; i < 10; ++i) s += std::string(";AC_") + POPS[i] + "=5";
  return *has_af ? s + ";AF=0.5" : s;
}
// record i of R against the splitter: field offsets, QUAL and AF spans, mask, the line
void check_long(const Result& R, uint64_t i, const std::string& line, uint32_t mask, const std::string& what) {
  const std::vector<std::string> f = split(line, '\t');
  if (f.size() < 8) { fail(what + ": the case has no eight fields"); return; }
  uint32_t fo[8], p = 0;
  for (int k = 0; k < 8; ++k) { fo[k] = p; p += (uint32_t)f[k].size() + 1; }
  for (int k = 0; k < 8; ++k)
    if (R.fo[i * 8 + k] != fo[k]) fail(what + ": field " + std::to_string(k) + " at " + std::to_string(R.fo[i * 8 + k]) + ", expected " + std::to_string(fo[k]));
  if (R.qs[i * 2] != fo[5] || R.qs[i * 2 + 1] != f[5].size()) fail(what + ": QUAL span");
  const uint32_t n_alt = (uint32_t)split(f[4], ',').size();
  std::string af;
  uint32_t a0 = n_alt, a1 = 0xffffffffu, q = fo[7];
  for (const std::string& e : split(f[7], ';')) {
    if (e.rfind("AF=", 0) == 0) { a0 = q + 3; a1 = (uint32_t)e.size() - 3; af = e.substr(3); break; }
    q += (uint32_t)e.size() + 1;
  }
  if (R.as[i * 2] != a0 || R.as[i * 2 + 1] != a1) fail(what + ": AF span " + std::to_string(R.as[i * 2]) + ", expected " + std::to_string(a0));
  if (a1 == 0xffffffffu)
    for (uint32_t a = 0; a < n_alt; ++a) af += a ? ",0.0" : "0.0";
  else if (af != "0.5") { fail(what + ": the case's AF is not 0.5"); return; }
  const std::string want = f[0] + "\t" + f[1] + "\t" + f[2] + "\t" + f[3] + "\t" + f[4] + "\t.\t" + (f[6] == "." ? "" : f[6]) + "\tAF=" + af + "\tGT" + gts(mask);
  if (R.flags[i] != 0 || R.mask[i] != mask || line_of(R, i) != want) fail(what + ": flags, mask or line");
}
}  // namespace

int main() {
  const Keys K = pop_keys();
  uint64_t records = 0;
  // ---- the key at every offset around the sweep, its value across it
  {
    const std::string head = "chr21\t100\t.\tA\tG\t.\tPASS\t";
    for (const char* value : {"5", "0,0,0,0,5", "0"}) {
      std::vector<std::string> lines;
      for (uint32_t o = 4075; o <= 4100; ++o) {
        std::string l = head + "pad=" + std::string(o - head.size() - 5, 'x') + ";AC_afr=" + value + ";";
        for (int i = 1; i < 10; ++i) l += std::string("AC_") + POPS[i] + "=0;";
        lines.push_back(l + "AF=0.25");
      }
      const Result R = run(lines, {}, K, 1);
      if (R.rc != HAWK_OK || R.n_kept != lines.size()) { fail("sweep seams"); continue; }
      for (uint64_t i = 0; i < lines.size(); ++i)
        if (line_of(R, i) != "chr21\t100\t.\tA\tG\t.\tPASS\tAF=0.25\tGT" + gts(std::string(value) == "0" ? 0 : 1)) fail("sweep seam line " + std::to_string(i));
      records += lines.size();
    }
  }
  // ---- whole-record lengths, the shortest record, the key first / last with every line end
  {
    std::vector<std::string> lines, ends;
    for (uint32_t length : {4095u, 4096u, 4097u, 12289u, 70001u})
      for (int at_end = 0; at_end < 2; ++at_end) {
        std::string l = record(at_end ? "" : "AC_afr=7", "0", "", ";pad=");
        l += std::string(length - 1 - l.size() - (at_end ? 9 : 0), 'y');
        if (at_end) l += ";AC_afr=7";
        lines.push_back(l); ends.push_back(at_end ? "\r\n" : "\n");
      }
    for (const char* tail : {"", "\tninth", "\t"})
      for (const char* e : {"\n", "\r\n"}) {
        lines.push_back(record("AC_afr=3", "0", "", "", "PASS", "G", "1", "AF=1") + tail); ends.push_back(e);
        lines.push_back(record("", "0", "", ";AC_afr=3") + tail); ends.push_back(e);
        lines.push_back("1\t1\t.\tA\tG\t.\t.\tAC_afr=1;AC_ami=1;AC_amr=1;AC_asj=1;AC_eas=1;AC_fin=1;AC_nfe=1;AC_mid=1;AC_sas=1;AC_remaining=1" + std::string(tail));
        ends.push_back(e);
      }
    const Result R = run(lines, ends, K, 1);
    if (R.rc != HAWK_OK || R.n_kept != lines.size()) fail("lengths and line ends");
    else
      for (uint64_t i = 0; i < lines.size(); ++i) {
        const std::string l = line_of(R, i);
        const bool shortest = lines[i][0] == '1';
        if (R.mask[i] != (shortest ? 0x3ffu : 1u) || l.size() < 40 || l.back() != '\n' || l.find('\r') != std::string::npos) fail("line " + std::to_string(i));
        if (shortest && l != "1\t1\t.\tA\tG\t.\t\tAF=0.0\tGT" + gts(0x3ff)) fail("shortest record");
      }
    records += lines.size();
  }
  // ---- values, decoys and flags
  {
    struct Case { std::string line; uint32_t flags_keep, flags_nokeep, mask; };
    const std::vector<Case> cases = {
        {record("AC_afr=0", "0"), 0, 0, 0}, {record("AC_afr=00", "0"), 0, 0, 0}, {record("AC_afr=5", "0"), 0, 0, 1}, {record("AC_afr=0,0,5", "0"), 0, 0, 1},
        {record("AC_afr=-3", "0"), 0, 0, 0}, {record("AC_afr=2147483647", "0"), 0, 0, 1}, {record("AC_afr=3,.", "0"), 0, 0, 1}, {record("AC_afr=+2", "0"), 0, 0, 1},
        {record("AC_afr=.", "0"), 4, 4, 0}, {record("AC_afr=.,3", "0"), 4, 4, 0}, {record("AC_afr=", "0"), 4, 4, 0}, {record("AC_afr", "0"), 4, 4, 0},
        {record("AC_afr=1x", "0"), 4, 4, 0}, {record("AC_afr=12345678901", "0"), 4, 4, 0}, {record("AC_afr=0,", "0"), 4, 4, 0}, {record("", "0"), 2, 2, 0},
        {record("AC_afr=0", "0", "AC_afr_XX=5;XAC_afr=5;AC_joint_afr=5;nhomalt_afr=5;x=AC_afr=5;"), 0, 0, 0},
        {record("AC_afr=5", "0", "", ";AC_afr=0"), 0, 0, 1}, {record("AC_afr=0", "0", "", ";AC_afr=5"), 0, 0, 0},
        {record("AC_afr=.", "0", "", "", "AC0"), 4, 1, 0}, {record("AC_afr=5", "0", "", "", "AC0;PASS"), 0, 0, 1}, {record("AC_afr=5", "0", "", "", "PASSED"), 0, 1, 1},
        {record("AC_afr=5", "0", "", "", "."), 0, 1, 1}, {record("AC_afr=5", "0", "", "", "PASS", "."), 16, 16, 0}, {record("AC_afr=5", "0", "", "", "PASS", "G", "1e3"), 32, 32, 0},
        {record("AC_afr=5", "0", "", "", "PASS", "G", ""), 32, 32, 0}, {"chr21\t5\t.\tA\tG\t.\tPASS", 8, 8, 0}, {"x", 8, 8, 0},
    };
    for (int keep = 0; keep < 2; ++keep)
      for (const Case& c : cases) {
        const Result R = run({c.line}, {}, K, keep);
        const uint32_t want = keep ? c.flags_keep : c.flags_nokeep;
        if (R.rc != HAWK_OK || R.flags[0] != want || R.mask[0] != (want ? 0 : c.mask) || R.n_kept != (want ? 0u : 1u) || (want != 0) != (R.n_bytes == 0))
          fail("flags of " + c.line.substr(0, 60) + " keep " + std::to_string(keep) + ": " + std::to_string(R.flags[0]));
        ++records;
      }
    // AF absent with 1, 2 and 3 ALT alleles; "." and lists
    const Result R = run({record("AC_afr=1", "0", "", "", "PASS", "G", "7", "AF_joint=0.5"), record("AC_afr=1", "0", "", "", "PASS", "G,T", "7", "AF_joint=0.5"),
                          record("AC_afr=1", "0", "", "", "PASS", "G,T,AC", "7", "AF_joint=0.5"), record("AC_afr=1", "0", "", "", "PASS", "G", "7", "AF=."),
                          record("AC_afr=1", "0", "", "", "PASS", "G", "7", "AF=0.5,."), record("AC_afr=1", "0", "", "", "PASS", "G", "7", "AF=0.125,1e-05,3")}, {}, K, 1);
    const char* afs[6] = {"AF=0.0\t", "AF=0.0,0.0\t", "AF=0.0,0.0,0.0\t", "AF=None\t", "AF=0.5,None\t", "AF=0.125,9.999999747378752e-06,3.0\t"};
    for (int i = 0; i < 6; ++i)
      if (R.rc != HAWK_OK || line_of(R, i).find(afs[i]) == std::string::npos) fail(std::string("AF case ") + afs[i]);
  }
  // ---- long fields: every field start at 4095 / 4096 / 4097, 5000 alleles, a 100 000-byte ALT
  {
    std::vector<std::string> lines, names;
    for (int f = 1; f <= 7; ++f)
      for (size_t o : {4095u, 4096u, 4097u}) {
        bool has_af;
        lines.push_back(long_record(f, o, &has_af));
        names.push_back("field " + std::to_string(f) + " at " + std::to_string(o));
        if (split(lines.back(), '\t').size() != 8 || lines.back()[o - 1] != '\t') fail(names.back() + ": not built so");
        lines.push_back(lines.back() + "\tAC_afr=5;AF=0.9");  // a ninth field the scan must not read
        names.push_back(names.back() + ", a ninth field");
      }
    std::string many;
    for (int a = 0; a < 5000; ++a) many += std::string(a ? "," : "") + (a % 3 == 0 ? "G" : a % 3 == 1 ? "TA" : "CAT");
    for (const std::string& alt : {many, rep("ACGT", 100000)}) {
      std::string s = "1\t1\t.\tA\t" + alt + "\t.\tPASS\tAC_afr=0";
      for (int i = 1; i < 10; ++i) s += std::string(";AC_") + POPS[i] + "=5";
      lines.push_back(s);
      names.push_back("ALT of " + std::to_string(alt.size()) + " bytes");
    }
    const Result R = run(lines, {}, K, 0);
    if (R.rc != HAWK_OK || R.n_kept != lines.size()) fail("long fields");
    else
      for (uint64_t i = 0; i < lines.size(); ++i) check_long(R, i, lines[i], 0x3fe, names[i]);
    records += lines.size();
  }
  // ---- refused arguments: nothing written
  {
    const std::string l = record("AC_afr=1", "0") + "\n";
    std::vector<uint8_t> text(l.begin(), l.end());
    const uint64_t lo[2] = {0, text.size()}, lo_long[2] = {0, text.size() + 1}, lo_mid[2] = {0, 9};
    Keys many, semi, eq, tab, empty;
    for (int i = 0; i < 32; ++i) many.add("K" + std::to_string(i));
    semi.add("a;b"); eq.add("a=b"); tab.add("a\tb"); empty.off.push_back(0);
    struct Bad { const char* what; const uint8_t* t; uint64_t tl; const uint64_t* lo; const Keys* k; };
    std::vector<uint8_t> cut(text.begin(), text.end() - 1);
    const Bad bad[] = {{"32 keys", text.data(), text.size(), lo, &many}, {"';' in a key", text.data(), text.size(), lo, &semi}, {"'=' in a key", text.data(), text.size(), lo, &eq},
                       {"tab in a key", text.data(), text.size(), lo, &tab}, {"empty key", text.data(), text.size(), lo, &empty}, {"no final newline", cut.data(), cut.size(), lo, &K},
                       {"line beyond the text", text.data(), text.size(), lo_long, &K}, {"line end inside a line", text.data(), text.size(), lo_mid, &K}};
    for (const Bad& b : bad) {
      uint32_t mask = 77, fo[8], sp[4] = {77, 77, 77, 77};
      uint8_t flags = 77;
      uint64_t nb = 77, nk = 77;
      for (uint32_t& f : fo) f = 77;
      const int rc = hawk_host_gnomad_lines(b.t, b.tl, b.lo, 1, b.k->blob.data(), b.k->off.data(), (uint32_t)b.k->off.size() - 1, 1, &mask, &flags, fo, sp, sp + 2,
                                            nullptr, nullptr, nullptr, 0, nullptr, &nb, &nk);
      if (rc != HAWK_E_INVALID || mask != 77 || flags != 77 || fo[0] != 77 || sp[0] != 77 || nb != 77 || nk != 77) fail(std::string("accepted: ") + b.what);
    }
    uint64_t nb = 77, nk = 77;
    if (hawk_host_gnomad_lines(nullptr, 0, nullptr, 0, K.blob.data(), K.off.data(), 10, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                               nullptr, &nb, &nk) != HAWK_OK || nb != 0 || nk != 0)
      fail("n_lines = 0");
  }
  // ---- float texts
  {
    struct F { const char* in; const char* out; };
    const F fs[] = {{"0", "0.0"}, {"-0.0", "-0.0"}, {"1e-4", "9.999999747378752e-05"}, {"1e-5", "9.999999747378752e-06"}, {"1e15", "999999986991104.0"},
                    {"1e16", "1.0000000272564224e+16"}, {"1234", "1234.0"}, {"0.1", "0.10000000149011612"}, {"0.5", "0.5"}, {"1e-45", "1.401298464324817e-45"},
                    {"3.4028235e38", "3.4028234663852886e+38"}, {"16777216", "16777216.0"}, {"1e39", nullptr}, {"nan", nullptr}, {"abc", nullptr}, {"", nullptr},
                    {"1,,2", nullptr}, {"0x10", nullptr}, {" 1", nullptr}};
    for (const F& f : fs) {
      std::vector<uint8_t> t(f.in, f.in + strlen(f.in));  // exactly the bytes
      const uint64_t start = 0;
      const uint32_t len = (uint32_t)t.size();
      uint64_t off[2] = {77, 77};
      uint8_t st = 77;
      uint8_t out[64];
      const int rc = hawk_host_f32_repr(t.data(), &start, &len, 1, ".", out, sizeof(out), off, &st, 1);
      const std::string got(out, out + off[1]);
      if (rc != HAWK_OK || (f.out ? (st != 0 || got != f.out) : (st != 1 || off[1] != 0))) fail(std::string("f32 text of '") + f.in + "': '" + got + "'");
    }
  }
  printf("gnomad check: %llu records, %d failures\n", (unsigned long long)records, failures);
  return failures ? 1 : 0;
}
