// DeviceSampling.h -- the random steps of the tools taken from the device's seeded draws
// (ife_random_rois, ife_sample_positions) and the gather of a list of boxes (ife_extract_rois);
// include/ife_hip.h states the draw.  What itk::RegionOfInterestGenerator<TMask>::generate gives
// with its host rejection loop, randomRegions gives for a mask that only the device walks:
//
//   std::vector<std::vector<Region>> r = randomRegions(mask, values, perValue, size, n, seed, stream);
//   std::vector<int64_t> p = randomPositions(mask, values, n, seed, stream);
//   std::vector<Pixel> v = extractRegions(image, rois);     // [roi][z][y][x]
//
// values empty: one set, mask != 0; perValue false: one set, mask in values; perValue true: one
// set per value, drawn from stream + its place.  Errors are thrown as itk::ExceptionObject; a set
// without a voxel that admits the box is one (the reference would draw forever).
#ifndef __DeviceSampling_h
#define __DeviceSampling_h

#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ife/Host/Engine.h"

namespace ife {
namespace host {

// IFE_DEVICE_SAMPLING (unset, empty or "0": off): MakeBag, MakeBagOnlyIntensity and the sampled
// branch of DetermineHistogramBinEdges take their boxes and positions from the device's draws.
inline bool DeviceSamplingFromEnvironment() {
  const char *v = std::getenv("IFE_DEVICE_SAMPLING");
  return v && v[0] && std::strcmp(v, "0") != 0;
}

// IFE_SEED fixes the seed, as for the host generators; unset, it comes from std::random_device.
inline uint64_t SamplingSeed() {
  if (const char *seed = std::getenv("IFE_SEED")) return std::strtoull(seed, nullptr, 10);
  std::random_device rd;
  return ((uint64_t)rd() << 32) | (uint64_t)rd();
}

template <typename TMask>
std::vector<std::vector<typename TMask::RegionType> > randomRegions(const TMask *mask, const std::vector<int> &values,
                                                                    bool perValue,
                                                                    const typename TMask::SizeType &size,
                                                                    size_t numberOfROIs, uint64_t seed,
                                                                    uint32_t stream) {
  typedef typename TMask::RegionType RegionType;
  const char *where = "randomRegions";
  if (!mask) throw itk::ExceptionObject("an input is missing", where);
  const ife_volume_desc d = describe(*mask);
  const int64_t boxSize[3] = {(int64_t)size[0], (int64_t)size[1], (int64_t)size[2]};
  const size_t sets = perValue ? values.size() : 1;
  std::vector<int64_t> boxes(6 * sets * numberOfROIs), counts(sets ? sets : 1);
  Engine &e = Engine::Instance();
  e.check(ife_random_rois(e.ctx(), mask->GetBufferPointer(), MaskDType<typename TMask::PixelType>::value, &d,
                          values.data(), (int)values.size(), perValue ? 1 : 0, boxSize, seed, stream, 0,
                          (int64_t)numberOfROIs, boxes.data(), counts.data(), IFE_MEM_HOST),
          where);
  std::vector<std::vector<RegionType> > rois(sets);
  for (size_t j = 0; j < sets; ++j)
    for (size_t i = 0; i < numberOfROIs; ++i) {
      const int64_t *q = &boxes[6 * (j * numberOfROIs + i)];
      typename RegionType::IndexType start;
      typename RegionType::SizeType extent;
      for (int k = 0; k < 3; ++k) {
        start[k] = q[k];
        extent[k] = (uint64_t)q[3 + k];
      }
      rois[j].push_back(RegionType(start, extent));
    }
  return rois;
}

// n linear indices of voxels whose label is one of values (the union), drawn from `stream`
template <typename TMask>
std::vector<int64_t> randomPositions(const TMask *mask, const std::vector<int> &values, size_t n, uint64_t seed,
                                     uint32_t stream) {
  const char *where = "randomPositions";
  if (!mask) throw itk::ExceptionObject("an input is missing", where);
  const ife_volume_desc d = describe(*mask);
  std::vector<int64_t> positions(n);
  int64_t count = 0;
  Engine &e = Engine::Instance();
  e.check(ife_sample_positions(e.ctx(), mask->GetBufferPointer(), MaskDType<typename TMask::PixelType>::value, &d,
                               values.data(), (int)values.size(), 0, nullptr, seed, stream, 0, (int64_t)n,
                               positions.data(), &count, IFE_MEM_HOST),
          where);
  return positions;
}

// itk::RegionOfInterestImageFilter over a list of boxes of one size: [roi][z][y][x]
template <typename TImage>
std::vector<typename TImage::PixelType> extractRegions(const TImage *image,
                                                       const std::vector<typename TImage::RegionType> &rois) {
  const char *where = "extractRegions";
  if (!image) throw itk::ExceptionObject("an input is missing", where);
  std::vector<typename TImage::PixelType> out;
  if (rois.empty()) return out;
  const ife_volume_desc d = describe(*image);
  std::vector<int64_t> boxes;
  boxes.reserve(6 * rois.size());
  for (const typename TImage::RegionType &roi : rois)
    for (int k = 0; k < 6; ++k) boxes.push_back(k < 3 ? (int64_t)roi.GetIndex()[k] : (int64_t)roi.GetSize()[k - 3]);
  for (int k = 0; k < 3; ++k)  // before anything is sized by the first box; the library checks the rest
    if (rois[0].GetSize()[k] > image->GetLargestPossibleRegion().GetSize()[k])
      throw itk::ExceptionObject("the first region is larger than the image", where);
  out.resize(rois.size() * (size_t)rois[0].GetNumberOfPixels());
  Engine &e = Engine::Instance();
  e.check(ife_extract_rois(e.ctx(), image->GetBufferPointer(), (int)sizeof(typename TImage::PixelType), &d,
                           boxes.data(), (int64_t)rois.size(), out.data(), IFE_MEM_HOST),
          where);
  return out;
}

}  // namespace host
}  // namespace ife

#endif
