// DeviceCoverage.h -- the two questions of the reference's tools/ImageBrowser.cxx asked of a volume
// that lies on the device (ife_value_census_f32, ife_threshold_mask, ife_random_rois,
// ife_roi_coverage; include/ife_hip.h states them):
//
//   ife::host::DeviceVolume vol(image);                      // uploaded once
//   ife::host::Census c = vol.census();                      // distinct values, their counts, the NaNs left out
//   ife::host::Coverage v = vol.coverage(size, low, high, ends, seed);
//
// coverage thresholds the volume into a byte mask, draws ends.back() boxes of `size` around voxels
// of the mask in one call (draws [0, n) are the rounds one after the other) and counts, per round,
// the voxels the boxes so far visit and how many of them lie in the mask.  Nothing but the counts
// leaves the device.  Errors are thrown as itk::ExceptionObject; a threshold range without a voxel
// that admits a box is one (the reference would draw forever).
#ifndef __DeviceCoverage_h
#define __DeviceCoverage_h

#include <cstdint>
#include <vector>

#include "ife/Host/Engine.h"

namespace ife {
namespace host {

struct Census {
  std::vector<float> values;      // ascending; -0 and +0 are one value, +0
  std::vector<uint32_t> counts;   // how often each occurs
  int64_t nan = 0;                // NaN elements, left out
};

struct Coverage {
  std::vector<int64_t> visited, hits;  // per round
  int64_t regionSize = 0;              // voxels between the thresholds
};

// bytes on the Engine's device, freed with their owner (ife_device_alloc)
class DeviceBytes {
 public:
  DeviceBytes() {}
  ~DeviceBytes() { reset(); }
  void reset() {
    if (p_) ife_device_free(Engine::Instance().ctx(), p_);
    p_ = nullptr;
  }
  void *alloc(size_t bytes, const char *where) {
    Engine &e = Engine::Instance();
    reset();
    e.check(ife_device_alloc(e.ctx(), bytes, &p_), where);
    return p_;
  }
  void *get() const { return p_; }

 private:
  DeviceBytes(const DeviceBytes &);
  DeviceBytes &operator=(const DeviceBytes &);
  void *p_ = nullptr;
};

class DeviceVolume {
 public:
  explicit DeviceVolume(const itk::Image<float, 3> &image)
      : desc_(describe(image)), n_((int64_t)image.GetLargestPossibleRegion().GetNumberOfPixels()) {
    const char *where = "DeviceVolume";
    if (n_ <= 0) throw itk::ExceptionObject("the image is empty", where);
    Engine &e = Engine::Instance();
    e.check(ife_device_upload(e.ctx(), image_.alloc((size_t)n_ * sizeof(float), where), image.GetBufferPointer(),
                              (size_t)n_ * sizeof(float)),
            where);
  }

  Census census() {
    const char *where = "DeviceVolume::census";
    Engine &e = Engine::Instance();
    Census c;
    int64_t n_unique = 0;
    e.check(ife_value_census_f32(e.ctx(), (const float *)image_.get(), n_, nullptr, nullptr, 0, &n_unique, &c.nan,
                                 IFE_MEM_DEVICE),
            where);
    if (n_unique == 0) return c;
    DeviceBytes uniq, counts;
    uniq.alloc((size_t)n_unique * 4, where);
    counts.alloc((size_t)n_unique * 4, where);
    e.check(ife_value_census_f32(e.ctx(), (const float *)image_.get(), n_, (float *)uniq.get(),
                                 (uint32_t *)counts.get(), n_unique, &n_unique, &c.nan, IFE_MEM_DEVICE),
            where);
    c.values.resize((size_t)n_unique);
    c.counts.resize((size_t)n_unique);
    download(c.values.data(), uniq.get(), n_unique, where);
    download(c.counts.data(), counts.get(), n_unique, where);
    return c;
  }

  // size: of every box; roundEnds: cumulative box counts, non-decreasing
  Coverage coverage(const int64_t size[3], float low, float high, const std::vector<int64_t> &roundEnds, uint64_t seed) {
    const char *where = "DeviceVolume::coverage";
    if (roundEnds.empty()) throw itk::ExceptionObject("no rounds", where);
    Engine &e = Engine::Instance();
    Coverage v;
    DeviceBytes mask, rois;
    mask.alloc((size_t)n_, where);
    e.check(ife_threshold_mask(e.ctx(), (const float *)image_.get(), n_, low, high, (uint8_t *)mask.get(),
                               &v.regionSize, IFE_MEM_DEVICE),
            where);
    const int64_t n_rois = roundEnds.back();
    rois.alloc((size_t)(n_rois > 0 ? n_rois : 1) * 6 * sizeof(int64_t), where);
    int64_t admissible = 0;
    e.check(ife_random_rois(e.ctx(), mask.get(), IFE_U8, &desc_, nullptr, 0, 0, size, seed, 0, 0, n_rois,
                            (int64_t *)rois.get(), &admissible, IFE_MEM_DEVICE),
            where);
    v.visited.resize(roundEnds.size());
    v.hits.resize(roundEnds.size());
    e.check(ife_roi_coverage(e.ctx(), mask.get(), IFE_U8, &desc_, (const int64_t *)rois.get(), n_rois,
                             roundEnds.data(), (int)roundEnds.size(), v.visited.data(), v.hits.data(), nullptr,
                             IFE_MEM_DEVICE),
            where);
    return v;
  }

 private:
  // n elements of four bytes from the device.  The library has no plain device-to-host copy: this is
  // ife_extract_region's crop of a one-row volume to itself, so n (here n_unique) is bound by that
  // call's axis length of 2^31-1, which the census' own limit of 2^31-1 elements keeps it below.
  static void download(void *dst, const void *src, int64_t n, const char *where) {
    Engine &e = Engine::Instance();
    ife_volume_desc row;
    row.nx = n; row.ny = 1; row.nz = 1;
    row.sx = row.sy = row.sz = 1.0;
    const int64_t whole[6] = {0, 0, 0, n, 1, 1};
    e.check(ife_extract_region(e.ctx(), src, 4, &row, whole, 0, nullptr, dst, IFE_MEM_DEVICE, IFE_MEM_HOST), where);
  }

  ife_volume_desc desc_;
  int64_t n_;
  DeviceBytes image_;
};

}  // namespace host
}  // namespace ife

#endif
