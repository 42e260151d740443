// The host half of a resident layer's index when the GPU ran ClassifyPath and Required
// (tarrequired.h): one layer's file records, its path blob and its counts come in, the
// TarIndexData IndexTarEntries would have built comes out.  Plain C++: it runs without HIP.
//
// The host touches only what the device asked: kReqAskAllow records get the exact allow
// rules (the masked ones, or all), kReqAskName records ClassifyPath and Required from the raw
// name -- which can add to the regular, whiteout and opaque counts and change or drop the
// path.  Both run through par in chunks.  When no record was dropped or renamed the blob is
// adopted as the pool as it stands; otherwise the kept paths are compacted.
//
// With skip options (skip != NULL: the device ran its skip stage, tarrequired.h) the records of the
// directories the device recorded (kReqSkipDir: fp, its rank in `start`) come along and are dropped
// from the index.  A kReqAskName entry is then finished in the host's order: a directory that a
// directory pattern matches means the device's under-decisions for later files lack a recorded
// directory -- the call returns 1 with nothing added to `out`, and the caller indexes the layer from
// the walk's records; a regular file goes through TarSkipEval, then TarSkipDirs::Under against the
// recorded directories, then Required.
#pragma once
#include <atomic>
#include <string>
#include <vector>

#include "tar_index_host.h"
#include "tarrequired.h"

namespace tsg {

struct TarRequiredHostStats {
  uint64_t ask_dropped = 0;  // asked records the host dropped
  TarSkipCounts skip;        // with skip options: the device's counts and the asked names' together
  bool adopted = false;      // the blob became the pool without a compaction
};

constexpr size_t kTarFileChunk = 256;

// allow_masked(path, len, rules) / allow_all(path, len): the scanner's AllowPathMasked / AllowPath;
// required(path, len, size): the analyzer's Required.  0, or -1 with the error set: a record points
// outside the blob, carries a verdict that has no record, or the counts contradict the records.
// 1 (with skip only): an asked name is a skipped directory; `out` is as it was.
template <class AllowMasked, class AllowAll, class Req, class Par = SerialFor>
int IndexTarFiles(const tsg_tar_file_rec* recs, uint64_t n_recs, const uint8_t* blob, uint64_t blob_bytes,
                  const TarRequiredCounts& cnt, AllowMasked&& allow_masked, AllowAll&& allow_all, Req&& required,
                  TarIndexData* out, Par&& par = Par(), TarRequiredHostStats* hs = nullptr,
                  const TarSkipOpts* skip = nullptr) {
  const uint64_t n_dirs = cnt.skipped_dirs();
  if (cnt.records != n_recs || cnt.path_bytes != blob_bytes || cnt.bad != 0 ||
      cnt.kept + cnt.ask_allow + cnt.ask_name + n_dirs != n_recs || (!skip && (cnt.pad[0] | cnt.pad[1]))) {
    SetError("tar files: the counts contradict the file records");
    return -1;
  }
  // the directories the device recorded, for the asked names (in walk order: the ranks ascend)
  TarSkipDirs skipped;
  if (skip && cnt.ask_name && n_dirs)
    for (uint64_t i = 0; i < n_recs; i++) {
      const tsg_tar_file_rec& r = recs[i];
      if (r.verdict != kReqSkipDir) continue;
      if (r.path_off > blob_bytes || uint64_t(r.path_len) + 1 > blob_bytes - r.path_off) break;  // (refused below)
      skipped.Record(std::string_view(reinterpret_cast<const char*>(blob + r.path_off), r.path_len), r.start);
    }
  const size_t n_chunks = (size_t(n_recs) + kTarFileChunk - 1) / kTarFileChunk;
  std::vector<uint8_t> keep(size_t(n_recs), 1);
  std::vector<std::string> renamed(cnt.ask_name ? size_t(n_recs) : 0);  // kReqAskName survivors' cleaned paths
  std::atomic<uint64_t> regular{0}, whiteouts{0}, opaque{0}, dropped{0}, dirs_seen{0}, sk_files{0}, sk_under{0};
  std::atomic<bool> bad{false}, asked_dir{false};
  par(n_chunks, [&](size_t c) {
    const size_t i1 = std::min(size_t(n_recs), (c + 1) * kTarFileChunk);
    for (size_t i = c * kTarFileChunk; i < i1; i++) {
      const tsg_tar_file_rec& r = recs[i];
      if (r.path_off > blob_bytes || uint64_t(r.path_len) + 1 > blob_bytes - r.path_off ||
          r.verdict < kReqKeep || (r.verdict > kReqAskName && !(skip && r.verdict == kReqSkipDir))) {
        bad.store(true);
        return;
      }
      if (r.verdict == kReqKeep) continue;
      if (r.verdict == kReqSkipDir) {  // recorded, not indexed
        keep[i] = 0;
        dirs_seen++;
        continue;
      }
      const char* p = reinterpret_cast<const char*>(blob + r.path_off);
      if (r.verdict == kReqAskAllow) {
        if (r.all_rules ? allow_all(p, uint64_t(r.path_len)) : allow_masked(p, uint64_t(r.path_len), r.rules)) {
          keep[i] = 0;
          dropped++;
        }
        continue;
      }
      TarEntry e;
      e.what = (r.typeflag == '0' || r.typeflag == '\0') ? 3 : 0;
      e.fp_off = r.path_off;  // a view of the blob, which stands in for the layer buffer of a kView source
      e.fp_len = r.path_len;
      ClassifyPath(r.typeflag, blob, &e);
      whiteouts += e.what == 1;
      opaque += e.what == 2;
      regular += e.what == 3;
      const std::string_view fp = e.path(blob);
      if (skip && (e.dir || e.what == 3)) {
        const uint8_t sk = TarSkipEval(*skip, e.dir, e.what == 3, fp);
        if (sk == kTarSkipDir) {
          asked_dir.store(true);
          return;
        }
        if (sk == kTarSkipFile || (e.what == 3 && skipped.Under(fp, r.start))) {
          (sk == kTarSkipFile ? sk_files : sk_under)++;
          keep[i] = 0;
          continue;
        }
      }
      if (e.what == 3 && required(fp.data(), uint64_t(fp.size()), int64_t(r.size))) {
        renamed[i].assign(fp.data(), fp.size());
      } else {
        keep[i] = 0;
        dropped++;
      }
    }
  });
  if (bad.load()) {
    SetError("tar files: a record has its path outside the path blob, or a verdict that has no record");
    return -1;
  }
  if (asked_dir.load()) return 1;
  if (dirs_seen.load() != n_dirs) {
    SetError("tar files: the counts contradict the file records");
    return -1;
  }
  const uint64_t asked_skipped = sk_files.load() + sk_under.load();
  if (skip) {
    out->skip.skipped_dirs += n_dirs;
    out->skip.skipped_files += cnt.skipped_files() + sk_files.load();
    out->skip.under_skipped_dir += cnt.under_skipped_dir() + sk_under.load();
    if (hs) hs->skip = TarSkipCounts{n_dirs, cnt.skipped_files() + sk_files.load(), cnt.under_skipped_dir() + sk_under.load()};
  }
  out->tar.entries += cnt.entries;
  out->tar.regular += cnt.regular + regular.load();
  out->tar.whiteouts += cnt.whiteouts + whiteouts.load();
  out->tar.opaque_dirs += cnt.opaque_dirs + opaque.load();
  if (hs) hs->ask_dropped = dropped.load() + asked_skipped;
  const size_t pool0 = out->pool.size(), files0 = out->files.size();
  if (dropped.load() == 0 && cnt.ask_name == 0 && n_dirs == 0) {  // the blob is the pool, the records are the files
    if (hs) hs->adopted = true;
    out->pool.append(reinterpret_cast<const char*>(blob), size_t(blob_bytes));
    out->files.resize(files0 + size_t(n_recs));
    par(n_chunks, [&](size_t c) {
      const size_t i1 = std::min(size_t(n_recs), (c + 1) * kTarFileChunk);
      for (size_t i = c * kTarFileChunk; i < i1; i++) {
        const tsg_tar_file_rec& r = recs[i];
        out->files[files0 + i] = TarIndexFile{pool0 + r.path_off, r.path_len, r.start, r.data, r.size};
      }
    });
    out->tar.required += n_recs;
    return 0;
  }
  // where each chunk's kept files and paths go
  std::vector<size_t> file_at(n_chunks + 1, 0), pool_at(n_chunks + 1, 0);
  par(n_chunks, [&](size_t c) {
    const size_t i1 = std::min(size_t(n_recs), (c + 1) * kTarFileChunk);
    size_t nf = 0, nb = 0;
    for (size_t i = c * kTarFileChunk; i < i1; i++) {
      if (!keep[i]) continue;
      nf++;
      nb += (recs[i].verdict == kReqAskName ? renamed[i].size() : size_t(recs[i].path_len)) + 1;
    }
    file_at[c + 1] = nf;
    pool_at[c + 1] = nb;
  });
  for (size_t c = 0; c < n_chunks; c++) {
    file_at[c + 1] += file_at[c];
    pool_at[c + 1] += pool_at[c];
  }
  out->pool.resize(pool0 + pool_at[n_chunks]);
  out->files.resize(files0 + file_at[n_chunks]);
  par(n_chunks, [&](size_t c) {
    const size_t i1 = std::min(size_t(n_recs), (c + 1) * kTarFileChunk);
    size_t f = files0 + file_at[c], at = pool0 + pool_at[c];
    for (size_t i = c * kTarFileChunk; i < i1; i++) {
      if (!keep[i]) continue;
      const tsg_tar_file_rec& r = recs[i];
      const bool own = r.verdict == kReqAskName;
      const char* p = own ? renamed[i].data() : reinterpret_cast<const char*>(blob + r.path_off);
      const size_t len = own ? renamed[i].size() : size_t(r.path_len);
      std::memcpy(&out->pool[at], p, len);
      out->pool[at + len] = '\0';
      out->files[f++] = TarIndexFile{at, len, r.start, r.data, r.size};
      at += len + 1;
    }
  });
  out->tar.required += file_at[n_chunks];
  return 0;
}

}  // namespace tsg
