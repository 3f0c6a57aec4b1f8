// lzf_check.cpp -- the LZF decoder of the compressed PCD route (csrc/nid_lzf_host.hpp) over untrusted bytes, as a stand-alone program
// for the address and undefined-behaviour sanitizers.  Host code only: it needs no GPU and must not be run on one.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I direct_visual_lidar_calibration_amd/csrc
//       tools/lzf_check.cpp -o lzf_check                      (one command line)
//   python tests/las_oracle.py --dump-lzf DIR                (the streams of tests/las_oracle.py as files)
//   ./lzf_check DIR/*.lzf
//
// Per file: the whole stream and every prefix of it, and `kMutations` seeded single-byte mutations, each decoded into heap buffers of
// several exact sizes -- the size the whole stream decodes to, one byte less, half, zero -- so that a write past the room given is a
// write past the allocation.  Every input must either decode or be refused with a reason, never write more than the room, and
// report what it wrote; the sanitizers abort on anything else.  Exit status 0 and a count per file when all held.
#include "nid_lzf_host.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

namespace {

constexpr int kMutations = 20000;
constexpr size_t kRoom = size_t(1) << 20;  // more than any of the test streams decodes to

struct Tally {
  long decoded = 0, refused = 0;
};

bool run(const std::vector<uint8_t>& bytes, size_t n, size_t room, Tally& t) {
  // copies of exactly n input bytes and exactly `room` output bytes on the heap: a read or write past either is past its allocation
  std::vector<uint8_t> exact(bytes.begin(), bytes.begin() + long(n)), out(room);
  size_t written = 0;
  std::string reason;
  const bool ok = nidlzf::decompress(exact.data(), exact.size(), out.data(), out.size(), written, reason);
  if (!ok && reason.empty()) {
    std::fprintf(stderr, "refused without a reason (%zu bytes into %zu)\n", n, room);
    return false;
  }
  if (written > room) {
    std::fprintf(stderr, "reports %zu bytes written into %zu\n", written, room);
    return false;
  }
  (ok ? t.decoded : t.refused)++;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s stream.lzf ...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; a++) {
    std::ifstream f(argv[a], std::ios::binary);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (bytes.empty()) {
      std::fprintf(stderr, "%s: empty or unreadable\n", argv[a]);
      return 2;
    }
    // what the whole stream decodes to, given room to spare (a stream that is refused still says how far it got)
    size_t full = 0;
    {
      std::vector<uint8_t> out(kRoom);
      std::string reason;
      nidlzf::decompress(bytes.data(), bytes.size(), out.data(), out.size(), full, reason);
    }
    const size_t rooms[] = {full, full ? full - 1 : 0, full / 2, 0, full + 7};
    Tally t;
    for (size_t n = 0; n <= bytes.size(); n++)
      for (const size_t room : rooms)
        if (!run(bytes, n, room, t)) return 1;
    uint64_t state = 0x9E3779B97F4A7C15ull ^ uint64_t(a);
    for (int m = 0; m < kMutations; m++) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      const size_t at = size_t((state >> 33) % bytes.size());
      const uint8_t value = uint8_t(state >> 24), old = bytes[at];
      bytes[at] = value;
      bool ok = true;
      for (const size_t room : rooms) ok = ok && run(bytes, bytes.size(), room, t);
      bytes[at] = old;
      if (!ok) return 1;
    }
    std::printf("%s: %zu bytes -> %zu, %zu prefixes, %d mutations, 5 buffer sizes each: %ld decoded, %ld refused\n", argv[a], bytes.size(), full, bytes.size() + 1, kMutations, t.decoded, t.refused);
  }
  return 0;
}
