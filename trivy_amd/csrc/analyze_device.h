// Analyze for HBM-resident files (tsg_analyzer_classify_device / _submit_device,
// analyze_device.cpp): the host half -- argument checks, Required and the
// binary gate's consequence per file, the scan paths, and what a pending
// submit owns -- apart from the GPU half (classify.h), so it runs without one.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "tsg_analyzer.h"

namespace tsg {

// What the library builds for a device submit; the scan borrows it, and it is
// freed with the tsg_pending (tsg_scan_wait).
struct DevicePlan {
  std::vector<uint8_t> kinds, binary;  // tsg_batch.transform / .binary
  std::string path_pool;               // the scan paths, packed ("/" prefix for image files)
  std::vector<uint64_t> path_off{0};
  std::vector<const char*> path_ptrs;
  std::vector<uint64_t> path_lens;
  std::vector<uint8_t> flags;          // the GPU's IsBinary flags
};

// The argument errors of tsg_device_files (tsg_analyzer.h), before any GPU work.
bool CheckDeviceFiles(const tsg_analyzer* a, const tsg_device_files* f, const char* who);
// Per file, from the binary flags: Required (path, size) false -> kind 3; flag
// set and not .pyc -> kind 3; flag set, .pyc -> kind 2, binary 1; else kind 1.
// st (optional): files, required, skipped_binary, pyc are filled.
void DeviceKinds(const tsg_analyzer* a, const tsg_device_files& f, const uint8_t* flags, uint8_t* kind,
                 uint8_t* binary, tsg_device_classify_stats* st);
// The GPU half (classify.h): flags[i] = IsBinary over file i's head, read from
// f.dev_arena at f.host_offsets (f.dev_offsets when given); only those fields
// and n_files are used.  On a pooled stream of its own; ms_kernel from HIP events.
bool ClassifyOnGpu(tsg_analyzer* a, const tsg_device_files& f, uint8_t* flags, double* ms_kernel, std::string* err);
// The scan paths: AnalysisInput.FilePath, with the "/" prefix when dir is "" (secret.go:130-135).
void BuildScanPaths(const tsg_device_files& f, DevicePlan* p);
// tsg_analyzer_submit_device with the flags given instead of computed on the
// GPU (host-half tests: the plan's lifetime across submit and wait).
int SubmitDeviceWithFlags(tsg_analyzer* a, const tsg_device_files* f, const uint8_t* flags, tsg_pending** out);

}  // namespace tsg
