// inflate_check_main.cpp - a stand-alone run of the host twin of the BGZF inflate (hawk_host_bgzf_inflate, hawk_hostutil.hip; the
// rules: hawk_inflate.h) for a sanitizer build: `make asan-inflate` compiles this file and hawk_hostutil.hip with
// -fsanitize=address,undefined and runs the program on tests/golden/bgzf_panel.bin, the panel of tests/bgzf_refs.py.  Every member
// alone in an input buffer of EXACTLY its size and a text buffer of EXACTLY its ISIZE (a byte read or written beyond either is a
// heap overflow the sanitizer sees), held to the status and the CRC32 of the text the panel names; the whole panel in one call on
// four threads; the refused arguments; then a few thousand corrupted members - bit flips, bytes overwritten, truncations, a wrong
// ISIZE - made from the panel's members, each again in buffers of exactly its sizes: whatever status they end in, they end.  The
// kernel runs the same header, so this is the evidence that a corrupt file cannot make either read or write out of bounds.
// Not part of the library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hawk.h"

namespace {
int failures = 0;
void fail(const std::string& what) { printf("FAILED: %s\n", what.c_str()); ++failures; }

struct PanelMember {
  std::vector<uint8_t> raw;
  uint32_t isize, crc, status;
};

uint32_t crc32_of(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}
uint32_t le32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

std::vector<PanelMember> read_panel(const char* path) {
  std::vector<PanelMember> out;
  FILE* f = fopen(path, "rb");
  if (!f) { fail(std::string("cannot open ") + path); return out; }
  std::vector<uint8_t> blob;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  if (blob.size() < 12 || memcmp(blob.data(), "BZPANEL1", 8) != 0) { fail("not a panel file"); return out; }
  const uint32_t n = le32(&blob[8]);
  size_t at = 12;
  for (uint32_t i = 0; i < n; ++i) {
    if (at + 16 > blob.size()) { fail("panel file cut short"); break; }
    PanelMember m;
    const uint32_t clen = le32(&blob[at]);
    m.isize = le32(&blob[at + 4]); m.crc = le32(&blob[at + 8]); m.status = blob[at + 12];
    at += 16;
    if (at + clen > blob.size()) { fail("panel file cut short"); break; }
    m.raw.assign(blob.begin() + at, blob.begin() + at + clen);
    at += clen;
    out.push_back(std::move(m));
  }
  return out;
}

// one member in heap blocks of exactly its sizes; returns its status, the text in *text
uint8_t run_alone(const std::vector<uint8_t>& raw, uint32_t isize, std::vector<uint8_t>* text, int* rc_out = nullptr) {
  uint8_t* in = (uint8_t*)malloc(raw.size() ? raw.size() : 1);
  uint8_t* out = (uint8_t*)malloc(isize ? isize : 1);
  if (raw.size()) memcpy(in, raw.data(), raw.size());
  const uint64_t c_off[2] = {0, raw.size()}, u_off[2] = {0, isize};
  uint8_t status = 0x77;
  const int rc = hawk_host_bgzf_inflate(in, raw.size(), c_off, u_off, 1, out, &status, 1);
  if ((rc == HAWK_OK) != (status == HAWK_BZ_OK)) fail("return code and status disagree");
  if (rc != HAWK_OK && rc != HAWK_E_INVALID) fail("a return code that is neither HAWK_OK nor HAWK_E_INVALID");
  if (status > HAWK_BZ_DISTANCE) fail("a status outside the enum");
  if (rc_out) *rc_out = rc;
  if (text) text->assign(out, out + isize);
  free(in);
  free(out);
  return status;
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t k) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % k;
}
}  // namespace

int main(int argc, char** argv) {
  const std::vector<PanelMember> panel = read_panel(argc > 1 ? argv[1] : "../../tests/golden/bgzf_panel.bin");
  if (panel.empty()) { fail("empty panel"); return 1; }
  // ---- every member alone
  size_t n_bad = 0;
  for (size_t i = 0; i < panel.size(); ++i) {
    const PanelMember& m = panel[i];
    std::vector<uint8_t> text;
    const uint8_t st = run_alone(m.raw, m.isize, &text);
    const std::string who = "member " + std::to_string(i);
    if (m.status == HAWK_BZ_OK) {
      if (st != HAWK_BZ_OK) fail(who + ": status " + std::to_string(st));
      else if (crc32_of(text.data(), text.size()) != m.crc) fail(who + ": text differs");
    } else {
      ++n_bad;
      if (st == HAWK_BZ_OK) fail(who + " must fail");
      else if (m.status != 255 && st != m.status) fail(who + ": status " + std::to_string(st) + ", expected " + std::to_string(m.status));
    }
  }
  // ---- the whole panel in one call on four threads, canaries around the text and every valid neighbour of a failed member intact
  {
    std::vector<uint8_t> in;
    std::vector<uint64_t> c_off{0}, u_off{64};
    for (const PanelMember& m : panel) {
      in.insert(in.end(), m.raw.begin(), m.raw.end());
      c_off.push_back(in.size());
      u_off.push_back(u_off.back() + m.isize);
    }
    std::vector<uint8_t> out(u_off.back() + 64, 0xA5), status(panel.size(), 0x77);
    const int rc = hawk_host_bgzf_inflate(in.data(), in.size(), c_off.data(), u_off.data(), (uint32_t)panel.size(), out.data(), status.data(), 4);
    if (rc != (n_bad ? HAWK_E_INVALID : HAWK_OK)) fail("whole panel: return code");
    for (size_t i = 0; i < 64; ++i)
      if (out[i] != 0xA5 || out[out.size() - 1 - i] != 0xA5) { fail("whole panel: a byte outside the text was written"); break; }
    for (size_t i = 0; i < panel.size(); ++i) {
      const bool ok = panel[i].status == HAWK_BZ_OK;
      if (ok != (status[i] == HAWK_BZ_OK)) fail("whole panel: status of member " + std::to_string(i));
      else if (ok && crc32_of(&out[u_off[i]], panel[i].isize) != panel[i].crc) fail("whole panel: text of member " + std::to_string(i));
    }
  }
  // ---- refused arguments: nothing is written
  {
    const PanelMember& m = panel[0];
    std::vector<uint8_t> out(m.isize + 1, 0xA5);
    uint8_t status = 0x77;
    const uint64_t c_ok[2] = {0, m.raw.size()}, u_ok[2] = {0, m.isize}, c_back[2] = {4, 0}, u_back[2] = {m.isize + 1ull, 0}, c_past[2] = {0, m.raw.size() + 1};
    auto refused = [&](const char* what, int rc) {
      if (rc != HAWK_E_INVALID) fail(std::string(what) + ": not refused");
      if (status != 0x77 || out[0] != 0xA5) fail(std::string(what) + ": something was written");
    };
    refused("descending c_off", hawk_host_bgzf_inflate(m.raw.data(), m.raw.size(), c_back, u_ok, 1, out.data(), &status, 1));
    refused("descending u_off", hawk_host_bgzf_inflate(m.raw.data(), m.raw.size(), c_ok, u_back, 1, out.data(), &status, 1));
    refused("member past in_bytes", hawk_host_bgzf_inflate(m.raw.data(), m.raw.size(), c_past, u_ok, 1, out.data(), &status, 1));
    refused("no c_off", hawk_host_bgzf_inflate(m.raw.data(), m.raw.size(), nullptr, u_ok, 1, out.data(), &status, 1));
    refused("no u_off", hawk_host_bgzf_inflate(m.raw.data(), m.raw.size(), c_ok, nullptr, 1, out.data(), &status, 1));
    refused("no input", hawk_host_bgzf_inflate(nullptr, m.raw.size(), c_ok, u_ok, 1, out.data(), &status, 1));
    if (hawk_host_bgzf_inflate(m.raw.data(), m.raw.size(), c_ok, u_ok, 1, out.data(), nullptr, 1) != HAWK_E_INVALID) fail("no status: not refused");
    if (hawk_host_bgzf_inflate(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 1) != HAWK_OK) fail("no members is HAWK_OK");
  }
  // ---- corrupted members: whatever they end in, they end, inside their buffers
  size_t n_corrupt = 0, n_still_ok = 0;
  for (int round = 0; round < 80; ++round) {
    for (size_t i = 0; i < panel.size(); ++i) {
      const PanelMember& m = panel[i];
      if (m.raw.size() > 40000 && round >= 8) continue;  // the large members a few times, the small ones often
      std::vector<uint8_t> raw = m.raw;
      uint32_t isize = m.isize;
      switch (rnd(5)) {
        case 0:  // bit flips
          for (uint32_t k = 0, n = 1 + rnd(4); k < n && !raw.empty(); ++k) raw[rnd((uint32_t)raw.size())] ^= (uint8_t)(1u << rnd(8));
          break;
        case 1:  // bytes overwritten
          for (uint32_t k = 0, n = 1 + rnd(8); k < n && !raw.empty(); ++k) raw[rnd((uint32_t)raw.size())] = (uint8_t)rnd(256);
          break;
        case 2:  // cut short, anywhere from nothing left to one byte missing
          raw.resize(rnd((uint32_t)raw.size()));
          break;
        case 3:  // the trailer kept, bytes taken out of the stream in front of it
          if (raw.size() > 30) raw.erase(raw.begin() + 18 + rnd((uint32_t)raw.size() - 26), raw.end() - 8);
          break;
        default:  // a wrong ISIZE, in the trailer and in the range given for the text
          isize = rnd(3) ? rnd(65537) : isize + 1 + rnd(3);
          if (raw.size() >= 4 && rnd(2)) { raw[raw.size() - 4] = (uint8_t)isize; raw[raw.size() - 3] = (uint8_t)(isize >> 8); raw[raw.size() - 2] = (uint8_t)(isize >> 16); raw[raw.size() - 1] = 0; }
          if (isize > 70000) isize = 70000;
          break;
      }
      n_still_ok += run_alone(raw, isize, nullptr) == HAWK_BZ_OK;
      ++n_corrupt;
    }
  }
  printf("inflate_check: %zu panel members (%zu malformed), %zu corrupted members (%zu still valid)%s\n", panel.size(), n_bad, n_corrupt, n_still_ok,
         failures ? "" : ": ok");
  return failures ? 1 : 0;
}
