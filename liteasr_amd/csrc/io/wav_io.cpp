// Native RIFF/WAVE reader (include/liteasr_io.h, the lasr_wav_* entries).
//
// The reference's pretraining path decodes every utterance with soundfile.read to float64 in
// Python, slices it, converts to float32 and pads in the collator
// (liteasr/dataclass/audio_data.py:30-33, liteasr/dataset/pretrain_dataset.py:51-56).  Here a
// minibatch's windows are read as they are stored, 16-bit PCM, straight into one caller-owned
// (typically pinned) int16 buffer on a few host threads; the division by 32768 happens on the
// device (csrc/prep.hip, lasr_pcm_to_float).
//
// Accepted: RIFF/WAVE, little endian, fmt tag 1 (PCM) or 0xFFFE (extensible) with the PCM
// sub-format, one channel, 16 bits.  Chunks before "data" are skipped (with the pad byte of an
// odd size); a data size of 0 or 0xFFFFFFFF means "to the end of the file", and a size beyond
// the file is clipped to it.  Everything else is an error that names the file.
#include "../../../include/liteasr_io.h"
#include "io_error.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

using lasr_io::fail;
using lasr_io::g_err;

struct WavInfo {
  int rate = 0, channels = 0, bits = 0;
  int64_t frames = 0, data_offset = 0;
};

// Up to n bytes at pos; returns how many were there (short at the end of the file).
int64_t pread_upto(int fd, void* dst, int64_t n, int64_t pos) {
  char* p = static_cast<char*>(dst);
  int64_t done = 0;
  while (done < n) {
    const ssize_t r = pread(fd, p + done, (size_t)(n - done), pos + done);
    if (r <= 0) break;
    done += r;
  }
  return done;
}

inline uint32_t le16(const unsigned char* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8); }
inline uint32_t le32(const unsigned char* b) { return le16(b) | (le16(b + 2) << 16); }

int wav_fail(const char* path, const std::string& why) { return fail(std::string("wav: ") + path + ": " + why); }

// KSDATAFORMAT_SUBTYPE_* tail: xxxx0000-0000-0010-8000-00aa00389b71 after the 2-byte format tag
const unsigned char kSubTail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};

int parse_wav(int fd, const char* path, WavInfo* w) {
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return wav_fail(path, "not a regular file");
  const int64_t fsize = st.st_size;
  unsigned char h[40];
  if (pread_upto(fd, h, 12, 0) != 12) return wav_fail(path, "truncated header (shorter than a RIFF header)");
  if (std::memcmp(h, "RIFF", 4) != 0 || std::memcmp(h + 8, "WAVE", 4) != 0)
    return wav_fail(path, "not a RIFF/WAVE file");
  bool have_fmt = false;
  int64_t pos = 12;
  for (;;) {
    if (pos > fsize - 8 || pread_upto(fd, h, 8, pos) != 8)
      return wav_fail(path, have_fmt ? "truncated: no data chunk" : "truncated: no fmt chunk");
    const uint32_t size = le32(h + 4);
    if (std::memcmp(h, "fmt ", 4) == 0) {
      if (size < 16) return wav_fail(path, "fmt chunk shorter than 16 bytes");
      const int64_t want = std::min<int64_t>(size, 40);
      if (pread_upto(fd, h, want, pos + 8) != want) return wav_fail(path, "truncated fmt chunk");
      uint32_t tag = le16(h);
      const uint32_t channels = le16(h + 2), rate = le32(h + 4), bits = le16(h + 14);
      if (tag == 0xFFFEu) {
        if (size < 40) return wav_fail(path, "extensible fmt chunk shorter than 40 bytes");
        if (std::memcmp(h + 26, kSubTail, 14) != 0) return wav_fail(path, "unknown extensible sub-format");
        tag = le16(h + 24);
      }
      if (tag == 3) return wav_fail(path, "IEEE-float samples (only 16-bit PCM is supported)");
      if (tag != 1) return wav_fail(path, "format tag " + std::to_string(tag) + " (only 16-bit PCM is supported)");
      if (channels != 1) return wav_fail(path, std::to_string(channels) + " channels (only mono is supported)");
      if (bits != 16) return wav_fail(path, std::to_string(bits) + "-bit samples (only 16-bit PCM is supported)");
      if (rate == 0 || rate > 0x7FFFFFFFu) return wav_fail(path, "bad sample rate");
      w->rate = (int)rate;
      w->channels = 1;
      w->bits = 16;
      have_fmt = true;
    } else if (std::memcmp(h, "data", 4) == 0) {
      if (!have_fmt) return wav_fail(path, "data chunk before the fmt chunk");
      const int64_t avail = fsize - (pos + 8);  // >= 0: the chunk header was read
      const int64_t bytes = (size == 0 || size == 0xFFFFFFFFu) ? avail : std::min<int64_t>(size, avail);
      w->data_offset = pos + 8;
      w->frames = bytes / 2;
      return 0;
    }
    pos += 8 + (int64_t)size + (size & 1u);
  }
}

// Samples [start, start + count) of an open file into out; what lies past the data is zero.
int read_window(int fd, const char* path, const WavInfo& w, int64_t start, int64_t count, int16_t* out,
                int64_t* got) {
  if (start < 0 || count < 0) return wav_fail(path, "negative start or count");
  int64_t n = start < w.frames ? std::min(count, w.frames - start) : 0;
  if (n > 0) {
    const int64_t r = pread_upto(fd, out, 2 * n, w.data_offset + 2 * start);
    n = r < 0 ? 0 : r / 2;  // the file shrank since it was probed: what is there
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
    for (int64_t i = 0; i < n; ++i) out[i] = (int16_t)__builtin_bswap16((uint16_t)out[i]);
#endif
  }
  if (count > n) std::memset(out + n, 0, sizeof(int16_t) * (size_t)(count - n));
  *got = n;
  return 0;
}

int open_ro(const char* path) { return ::open(path, O_RDONLY | O_CLOEXEC); }

}  // namespace

extern "C" int lasr_wav_probe(const char* path, int* rate, int* channels, int* bits, int64_t* frames,
                              int64_t* data_offset) {
  if (!path) return fail("lasr_wav_probe: null path");
  const int fd = open_ro(path);
  if (fd < 0) return wav_fail(path, "cannot open");
  WavInfo w;
  const int rc = parse_wav(fd, path, &w);
  ::close(fd);
  if (rc) return rc;
  if (rate) *rate = w.rate;
  if (channels) *channels = w.channels;
  if (bits) *bits = w.bits;
  if (frames) *frames = w.frames;
  if (data_offset) *data_offset = w.data_offset;
  return 0;
}

extern "C" int lasr_wav_read_i16(const char* path, int64_t start, int64_t count, int16_t* out, int64_t* got) {
  if (!path || (count > 0 && !out)) return fail("lasr_wav_read_i16: null argument");
  const int fd = open_ro(path);
  if (fd < 0) return wav_fail(path, "cannot open");
  WavInfo w;
  int64_t n = 0;
  int rc = parse_wav(fd, path, &w);
  if (!rc) rc = read_window(fd, path, w, start, count, out, &n);
  ::close(fd);
  if (rc) return rc;
  if (got) *got = n;
  return 0;
}

extern "C" int lasr_wav_read_batch(int n, const char* const* paths, const int64_t* starts, int64_t count,
                                   int16_t* out, int64_t* got, int nthreads) {
  if (n < 0 || count < 0 || (n > 0 && (!paths || !starts || !got || (count > 0 && !out))))
    return fail("lasr_wav_read_batch: bad argument");
  if (n == 0) return 0;
  for (int i = 0; i < n; ++i)
    if (!paths[i]) return fail("lasr_wav_read_batch: null path");
  if (nthreads <= 0) nthreads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  nthreads = std::min(std::min(nthreads, 16), n);
  std::atomic<int> next{0};
  std::atomic<int> bad{-1};
  std::vector<std::string> errs(nthreads);
  auto work = [&](int tid) {
    struct Open {
      int fd;
      WavInfo w;
    };
    std::unordered_map<std::string, Open> files;  // a recording shared by many segments stays open
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n || bad.load() >= 0) break;
      const std::string p(paths[i]);
      auto it = files.find(p);
      int rc = 0;
      if (it == files.end()) {
        Open o{open_ro(paths[i]), WavInfo()};
        if (o.fd < 0) {
          rc = wav_fail(paths[i], "cannot open");
        } else {
          rc = parse_wav(o.fd, paths[i], &o.w);
          if (rc) ::close(o.fd);
          else it = files.emplace(p, o).first;
        }
      }
      if (!rc) rc = read_window(it->second.fd, paths[i], it->second.w, starts[i], count, out + (int64_t)i * count, &got[i]);
      if (rc) {
        errs[tid] = g_err;
        bad.store(i);
        break;
      }
    }
    for (auto& kv : files) ::close(kv.second.fd);
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nthreads; ++t) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  if (bad.load() >= 0) {
    for (auto& e : errs)
      if (!e.empty()) return fail(e);
    return fail("lasr_wav_read_batch: failed");
  }
  return 0;
}
