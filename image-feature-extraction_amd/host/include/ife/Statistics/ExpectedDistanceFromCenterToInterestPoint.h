// ExpectedDistanceFromCenterToInterestPoint.h -- host mirror of the reference's function
// template of the same name (include/ife/Statistics/ExpectedDistanceFromCenterToInterestPoint.h:9-43):
//
//   double ed = expectedDistanceFromCenterToInterestPoint<MaskType, ImageType>(mask, prob);
//
// The signed Maurer distance map of the mask (inside positive, image spacing used), its product
// with the probability image and the mean over the mask all run on the device
// (ife_expected_distance); the map itself is never stored.  Only `mask != 0` matters (:35), so
// a mask of any pixel type is reduced to that as unsigned char here.  Errors are thrown as
// itk::ExceptionObject, as the filters of the reference do on Update() (:25).  The images are
// taken as plain pointers: a Pointer of this mirror converts to one, and so does what a
// reader's GetOutput() returns (the call of the reference's tool, :78, compiles unchanged).
#ifndef __ExpectedDistanceFromCenterToInterestPoint_h
#define __ExpectedDistanceFromCenterToInterestPoint_h

#include <vector>

#include "ife/Host/Engine.h"

template <typename TMask, typename TProbabilityImage>
double expectedDistanceFromCenterToInterestPoint(const TMask *objectMask, const TProbabilityImage *probImage) {
  const char *where = "expectedDistanceFromCenterToInterestPoint";
  if (!objectMask || !probImage) throw itk::ExceptionObject("an input is missing", where);
  ife::host::same_size(*objectMask, *probImage, where);
  const ife_volume_desc d = ife::host::describe(*objectMask);
  const size_t n = (size_t)(d.nx * d.ny * d.nz);
  const typename TMask::PixelType *m = objectMask->GetBufferPointer();
  std::vector<unsigned char> fg(n);
  for (size_t i = 0; i < n; ++i) fg[i] = m[i] != 0;
  const typename TProbabilityImage::PixelType *p = probImage->GetBufferPointer();
  const std::vector<double> prob(p, p + n);
  ife::host::Engine &e = ife::host::Engine::Instance();
  double result = 0.0;
  e.check(ife_expected_distance(e.ctx(), fg.data(), IFE_U8, prob.data(), &d, &result, nullptr, IFE_MEM_HOST),
          where);
  return result;
}

#endif
