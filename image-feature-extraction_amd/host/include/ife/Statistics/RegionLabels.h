// RegionLabels.h -- the label of every region of interest: the mode of an unsigned char label
// image inside the region's box, the loop of the reference's tools/ExtractLabels.cxx:164-212 as
// two calls (the rule, ties included, is stated in include/ife_hip.h above ife_roi_labels):
//
//   std::vector<unsigned char> l = regionLabels(image, rois, ignored, dominant);
//   std::vector<unsigned char> l = denseRegionLabels(image, genMask, size, ignored, dominant);
//
// The first takes a list of boxes (ife_roi_labels).  The second takes what DenseROIGenerator takes,
// a generating mask and a box size, and returns the labels of the generator's regions in their
// order without the boxes (ife_dense_roi_labels: sliding box counts on the device).  Errors are
// thrown as itk::ExceptionObject; a box that leaves the image is one, as the reference's region
// iterator throws there (:180-187).
#ifndef __RegionLabels_h
#define __RegionLabels_h

#include <vector>

#include "ife/Host/Engine.h"

template <typename TImage>
std::vector<unsigned char> regionLabels(const TImage *image, const std::vector<typename TImage::RegionType> &rois,
                                        const std::vector<int> &ignoredLabels, int dominantLabel) {
  const char *where = "regionLabels";
  if (!image) throw itk::ExceptionObject("an input is missing", where);
  const ife_volume_desc d = ife::host::describe(*image);
  std::vector<int64_t> boxes;
  boxes.reserve(6 * rois.size());
  for (const typename TImage::RegionType &roi : rois)
    for (int k = 0; k < 6; ++k) boxes.push_back(k < 3 ? (int64_t)roi.GetIndex()[k] : (int64_t)roi.GetSize()[k - 3]);
  std::vector<unsigned char> labels(rois.size());
  ife::host::Engine &e = ife::host::Engine::Instance();
  e.check(ife_roi_labels(e.ctx(), image->GetBufferPointer(), ife::host::MaskDType<typename TImage::PixelType>::value,
                         &d, boxes.data(), (int64_t)rois.size(), ignoredLabels.data(), (int)ignoredLabels.size(),
                         dominantLabel, labels.data(), IFE_MEM_HOST),
          where);
  return labels;
}

template <typename TImage, typename TMask>
std::vector<unsigned char> denseRegionLabels(const TImage *image, const TMask *genMask,
                                             const typename TImage::SizeType &size,
                                             const std::vector<int> &ignoredLabels, int dominantLabel) {
  const char *where = "denseRegionLabels";
  if (!image || !genMask) throw itk::ExceptionObject("an input is missing", where);
  ife::host::same_size(*image, *genMask, where);
  const ife_volume_desc d = ife::host::describe(*image);
  const int64_t boxSize[3] = {(int64_t)size[0], (int64_t)size[1], (int64_t)size[2]};
  const int imageType = ife::host::MaskDType<typename TImage::PixelType>::value;
  const int maskType = ife::host::MaskDType<typename TMask::PixelType>::value;
  ife::host::Engine &e = ife::host::Engine::Instance();
  int64_t count = 0, got = 0;
  e.check(ife_dense_roi_labels(e.ctx(), image->GetBufferPointer(), imageType, genMask->GetBufferPointer(), maskType,
                               &d, boxSize, ignoredLabels.data(), (int)ignoredLabels.size(), dominantLabel, nullptr, 0,
                               &count, IFE_MEM_HOST),
          where);
  std::vector<unsigned char> labels((size_t)count);
  if (count == 0) return labels;
  e.check(ife_dense_roi_labels(e.ctx(), image->GetBufferPointer(), imageType, genMask->GetBufferPointer(), maskType,
                               &d, boxSize, ignoredLabels.data(), (int)ignoredLabels.size(), dominantLabel,
                               labels.data(), count, &got, IFE_MEM_HOST),
          where);
  if (got != count) throw itk::ExceptionObject("the number of dense regions changed between two calls", where);
  return labels;
}

#endif
