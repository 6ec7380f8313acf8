// Host AddressSanitizer + UBSan driver of the native WAV reader (csrc/io/wav_io.cpp), compiled
// together with it (tools/asan/Makefile, target run-wav).  Every header variant the reader
// accepts or refuses, every truncation length of a valid file, and seeded single-byte mutations
// of the first 64 bytes go through lasr_wav_probe, lasr_wav_read_i16 and the threaded
// lasr_wav_read_batch; results of accepted files are checked against the bytes written.
// Usage: wav_check <scratch dir>.  Prints "wav sanitizer checks: clean" when nothing failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/liteasr_io.h"

namespace {

typedef std::vector<unsigned char> Bytes;
int g_failed = 0;

#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      std::fprintf(stderr, "CHECK failed (%s:%d): ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);               \
      std::fprintf(stderr, "\n");                      \
      ++g_failed;                                      \
    }                                                  \
  } while (0)

void put16(Bytes& b, uint32_t v) { b.push_back(v & 255); b.push_back((v >> 8) & 255); }
void put32(Bytes& b, uint32_t v) { put16(b, v & 0xFFFF); put16(b, v >> 16); }
void tag(Bytes& b, const char* t) { b.insert(b.end(), t, t + 4); }

void chunk(Bytes& b, const char* id, const Bytes& body, int64_t size = -1) {
  tag(b, id);
  put32(b, size < 0 ? (uint32_t)body.size() : (uint32_t)size);
  b.insert(b.end(), body.begin(), body.end());
  if (body.size() & 1) b.push_back(0);
}

Bytes fmt_body(uint32_t tagv, uint32_t ch, uint32_t rate, uint32_t bits, bool extensible = false, uint32_t sub = 1) {
  Bytes f;
  put16(f, extensible ? 0xFFFE : tagv);
  put16(f, ch);
  put32(f, rate);
  put32(f, rate * ch * bits / 8);
  put16(f, ch * bits / 8);
  put16(f, bits);
  if (extensible) {
    put16(f, 22);
    put16(f, bits);
    put32(f, 4);
    put16(f, sub);
    const unsigned char tail[14] = {0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71};
    f.insert(f.end(), tail, tail + 14);
  }
  return f;
}

std::vector<int16_t> samples(int n, uint32_t seed) {
  std::vector<int16_t> s(n);
  for (int i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    s[i] = (int16_t)(seed >> 16);
  }
  if (n > 2) { s[0] = -32768; s[1] = 32767; s[2] = 0; }
  return s;
}

Bytes pcm_bytes(const std::vector<int16_t>& s) {
  Bytes d;
  for (int16_t v : s) put16(d, (uint16_t)v);
  return d;
}

Bytes riff(const std::vector<std::pair<std::string, Bytes>>& chunks, int64_t data_size = -1) {
  Bytes b;
  tag(b, "RIFF");
  put32(b, 0);
  tag(b, "WAVE");
  for (auto& c : chunks) chunk(b, c.first.c_str(), c.second, c.first == "data" ? data_size : -1);
  const uint32_t total = (uint32_t)b.size() - 8;
  b[4] = total & 255; b[5] = (total >> 8) & 255; b[6] = (total >> 16) & 255; b[7] = (total >> 24) & 255;
  return b;
}

std::string write_file(const std::string& dir, const std::string& name, const Bytes& b) {
  const std::string p = dir + "/" + name;
  FILE* f = std::fopen(p.c_str(), "wb");
  if (!f) { std::perror(p.c_str()); std::exit(2); }
  if (!b.empty()) std::fwrite(b.data(), 1, b.size(), f);
  std::fclose(f);
  return p;
}

// All three entries on one file.  expect >= 0: must succeed with that many frames and these samples.
// expect == -1: must fail with a message naming the file.  expect == -2: either, but never a bad answer.
void exercise(const std::string& p, int64_t expect, const std::vector<int16_t>* want) {
  int rate = 0, ch = 0, bits = 0;
  int64_t frames = -1, off = -1;
  const int rc = lasr_wav_probe(p.c_str(), &rate, &ch, &bits, &frames, &off);
  if (expect >= 0) CHECK(rc == 0 && frames == expect, "%s: probe rc %d frames %lld (want %lld): %s", p.c_str(), rc,
                         (long long)frames, (long long)expect, rc ? lasr_io_last_error() : "");
  if (expect == -1) {
    const char* e = lasr_io_last_error();
    CHECK(rc < 0 && e && std::strstr(e, p.c_str()), "%s: expected an error naming the file, rc %d", p.c_str(), rc);
  }
  if (rc == 0) CHECK(ch == 1 && bits == 16 && rate > 0 && frames >= 0 && off >= 20, "%s: bad probe result", p.c_str());
  const int64_t n = rc == 0 ? frames : 16;
  // windows: whole, inside, across the end, at the end, empty
  const int64_t wins[][2] = {{0, n}, {0, n + 5}, {n / 2, n}, {n, 4}, {n + 3, 2}, {1, 0}, {0, 1}};
  for (auto& w : wins) {
    std::vector<int16_t> out((size_t)w[1] + 1, 0x5A5A);
    int64_t got = -1;
    const int r2 = lasr_wav_read_i16(p.c_str(), w[0], w[1], out.data(), &got);
    CHECK((r2 == 0) == (rc == 0), "%s: read_i16 and probe disagree", p.c_str());
    if (r2) continue;
    const int64_t there = w[0] < n ? std::min(w[1], n - w[0]) : 0;
    CHECK(got == there, "%s: window (%lld, %lld) got %lld want %lld", p.c_str(), (long long)w[0], (long long)w[1],
          (long long)got, (long long)there);
    CHECK(out[(size_t)w[1]] == 0x5A5A, "%s: wrote past the window", p.c_str());
    for (int64_t i = 0; i < w[1]; ++i) {
      const int16_t e = i < there ? (want ? (*want)[(size_t)(w[0] + i)] : out[(size_t)i]) : 0;
      if (out[(size_t)i] != e) { CHECK(false, "%s: sample %lld of window (%lld, %lld)", p.c_str(), (long long)i, (long long)w[0], (long long)w[1]); break; }
    }
  }
  for (int threads : {1, 4}) {
    const char* paths[5] = {p.c_str(), p.c_str(), p.c_str(), p.c_str(), p.c_str()};
    const int64_t starts[5] = {0, 1, n / 2, n, n + 7};
    const int64_t count = n / 2 + 3;
    std::vector<int16_t> out((size_t)(5 * count) + 1, 0x5A5A);
    int64_t got[5] = {-1, -1, -1, -1, -1};
    const int r3 = lasr_wav_read_batch(5, paths, starts, count, out.data(), got, threads);
    CHECK((r3 == 0) == (rc == 0), "%s: read_batch and probe disagree", p.c_str());
    if (r3) continue;
    CHECK(out[(size_t)(5 * count)] == 0x5A5A, "%s: batch wrote past its buffer", p.c_str());
    for (int k = 0; k < 5; ++k) {
      const int64_t there = starts[k] < n ? std::min(count, n - starts[k]) : 0;
      CHECK(got[k] == there, "%s: batch row %d got %lld want %lld", p.c_str(), k, (long long)got[k], (long long)there);
      for (int64_t i = 0; i < count; ++i) {
        const int16_t v = out[(size_t)(k * count + i)];
        const int16_t e = i < there ? (want ? (*want)[(size_t)(starts[k] + i)] : v) : 0;
        if (v != e) { CHECK(false, "%s: batch row %d sample %lld", p.c_str(), k, (long long)i); break; }
      }
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::vector<int16_t> s = samples(301, 7);
  const Bytes d = pcm_bytes(s);
  const Bytes plain = riff({{"fmt ", fmt_body(1, 1, 16000, 16)}, {"data", d}});

  // accepted variants
  exercise(write_file(dir, "plain.wav", plain), 301, &s);
  exercise(write_file(dir, "ext.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16, true)}, {"data", d}})), 301, &s);
  exercise(write_file(dir, "list.wav", riff({{"LIST", Bytes(26, 'x')}, {"fmt ", fmt_body(1, 1, 16000, 16)},
                                             {"fact", Bytes(4, 0)}, {"data", d}})), 301, &s);
  exercise(write_file(dir, "odd.wav", riff({{"fmt ", fmt_body(1, 1, 8000, 16)}, {"junk", Bytes(7, 'j')}, {"data", d}})),
           301, &s);
  exercise(write_file(dir, "ffff.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16)}, {"data", d}}, 0xFFFFFFFFll)), 301, &s);
  exercise(write_file(dir, "zero.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16)}, {"data", d}}, 0)), 301, &s);
  exercise(write_file(dir, "beyond.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16)}, {"data", d}}, 100000)), 301, &s);
  exercise(write_file(dir, "empty.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16)}, {"data", Bytes()}})), 0, &s);

  // refused variants
  exercise(write_file(dir, "u8.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 8)}, {"data", d}})), -1, nullptr);
  exercise(write_file(dir, "stereo.wav", riff({{"fmt ", fmt_body(1, 2, 16000, 16)}, {"data", d}})), -1, nullptr);
  exercise(write_file(dir, "float.wav", riff({{"fmt ", fmt_body(3, 1, 16000, 32)}, {"data", d}})), -1, nullptr);
  exercise(write_file(dir, "extfloat.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16, true, 3)}, {"data", d}})), -1, nullptr);
  exercise(write_file(dir, "short20.wav", Bytes(plain.begin(), plain.begin() + 20)), -1, nullptr);
  exercise(write_file(dir, "nonriff.wav", Bytes(200, 'A')), -1, nullptr);
  exercise(write_file(dir, "nodata.wav", riff({{"fmt ", fmt_body(1, 1, 16000, 16)}, {"LIST", Bytes(10, 'x')}})), -1, nullptr);
  exercise(write_file(dir, "datafirst.wav", riff({{"data", d}, {"fmt ", fmt_body(1, 1, 16000, 16)}})), -1, nullptr);
  exercise(dir + "/does_not_exist.wav", -1, nullptr);
  exercise(dir, -1, nullptr);  // a directory

  // every truncation length of a valid file with a chunk before fmt: fails cleanly up to the data
  // chunk's header, then succeeds with the samples that are there
  const Bytes listed = riff({{"LIST", Bytes(9, 'x')}, {"fmt ", fmt_body(1, 1, 16000, 16, true)}, {"data", d}});
  const size_t data_at = listed.size() - d.size();  // first sample byte (602 bytes: no pad byte)
  for (size_t len = 0; len <= listed.size(); ++len) {
    const std::string p = write_file(dir, "trunc.wav", Bytes(listed.begin(), listed.begin() + len));
    if (len < data_at) exercise(p, -1, nullptr);
    else exercise(p, std::min<int64_t>(301, (int64_t)(len - data_at) / 2), &s);
  }

  // seeded single-byte mutations of the first 64 bytes: any outcome but a wrong memory access
  uint32_t seed = 12345;
  for (int it = 0; it < 400; ++it) {
    seed = seed * 1664525u + 1013904223u;
    Bytes m = (it & 1) ? listed : plain;
    const size_t at = (seed >> 8) % 64;
    seed = seed * 1664525u + 1013904223u;
    m[at] = (unsigned char)(seed >> 16);
    exercise(write_file(dir, "mut.wav", m), -2, nullptr);
  }

  // bad arguments
  int64_t got = 0;
  int16_t one = 0;
  CHECK(lasr_wav_probe(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0, "null path accepted");
  const std::string pp = write_file(dir, "plain.wav", plain);
  CHECK(lasr_wav_probe(pp.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0, "null outputs refused");
  CHECK(lasr_wav_read_i16(pp.c_str(), -1, 1, &one, &got) < 0, "negative start accepted");
  CHECK(lasr_wav_read_i16(pp.c_str(), 0, -1, &one, &got) < 0, "negative count accepted");
  CHECK(lasr_wav_read_i16(pp.c_str(), 0, 1, &one, nullptr) == 0 && one == -32768, "got = NULL refused");
  CHECK(lasr_wav_read_batch(0, nullptr, nullptr, 4, nullptr, nullptr, 3) == 0, "empty batch refused");
  const char* two[2] = {pp.c_str(), "/nonexistent/x.wav"};
  const int64_t st[2] = {0, 0};
  int16_t buf[8];
  int64_t g2[2];
  CHECK(lasr_wav_read_batch(2, two, st, 4, buf, g2, 2) < 0 && std::strstr(lasr_io_last_error(), "/nonexistent/x.wav"),
        "batch with a missing file");
  CHECK(lasr_wav_read_batch(2, two, st, -4, buf, g2, 2) < 0, "negative batch count accepted");

  if (g_failed) {
    std::fprintf(stderr, "wav sanitizer checks: %d FAILED\n", g_failed);
    return 1;
  }
  std::printf("wav sanitizer checks: clean\n");
  return 0;
}
