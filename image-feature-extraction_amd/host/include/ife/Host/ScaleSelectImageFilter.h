// ScaleSelectImageFilter.h -- the maximum over scales of gamma-normalised measures of the Hessian
// eigenvalues (Laplacian, tube, plate, blob) and the scale that reached it, on the device
// (ife_scale_select; the arithmetic is defined in include/ife_hip.h).  Ours: the reference has no
// counterpart.  Eager, no pipeline; direction cosines are ignored.  float and short images with
// unsigned char and unsigned short masks go to the device; any other type does not compile: there
// is no CPU path.  The feature path follows the engine's context (IFE_DIFFERENTIAL).
#ifndef IFE_HOST_SCALESELECTIMAGEFILTER_H
#define IFE_HOST_SCALESELECTIMAGEFILTER_H

#include <vector>

#include "ife/Host/Engine.h"

namespace itk {

template <typename TImage, typename TMask>
class ScaleSelectImageFilter {
 public:
  typedef ScaleSelectImageFilter Self;
  typedef Image<float, 3> ResponseImageType;
  typedef Image<unsigned char, 3> ScaleImageType;
  ifeNewMacro(Self);
  void SetInputImage(const TImage *in) { in_ = in; dirty_ = true; }
  void SetInputMask(const TMask *mask) { mask_ = mask; dirty_ = true; }  // may stay unset: no mask
  void SetScales(const std::vector<float> &scales) { scales_ = scales; dirty_ = true; }
  void SetMeasures(const std::vector<ife_scale_measure> &measures) { measures_ = measures; dirty_ = true; }
  void AddMeasure(const ife_scale_measure &m) { measures_.push_back(m); dirty_ = true; }
  unsigned int GetNumberOfMeasures() const { return (unsigned int)measures_.size(); }
  void Update() {
    if (!dirty_) return;
    if (!in_) throw ExceptionObject("Input is required", "ScaleSelectImageFilter");
    if (mask_) ife::host::same_size(*in_, *mask_, "ScaleSelectImageFilter");
    ife::host::Engine &e = ife::host::Engine::Instance();
    const ife_volume_desc vol = ife::host::describe(*in_);
    const size_t n = (size_t)in_->GetLargestPossibleRegion().GetNumberOfPixels(), nm = measures_.size();
    std::vector<float> response(n * nm);
    std::vector<unsigned char> index(n * nm);
    ife_ctx *ctx = e.ctx();
    // the counts as they are: the library refuses what it does not take and names the argument
    e.check(ife_scale_select(ctx, in_->GetBufferPointer(), ife::host::ImageDType<typename TImage::PixelType>::value,
                             mask_ ? mask_->GetBufferPointer() : nullptr,
                             ife::host::MaskDType<typename TMask::PixelType>::value, &vol, scales_.data(),
                             (int)scales_.size(), measures_.data(), (int)nm, response.data(), index.data(),
                             IFE_MEM_HOST),
            "ScaleSelectImageFilter");
    responses_.assign(nm, ResponseImageType::Pointer());
    indices_.assign(nm, ScaleImageType::Pointer());
    for (size_t m = 0; m < nm; ++m) {  // the input's geometry goes with every output
      responses_[m] = ResponseImageType::New();
      responses_[m]->CopyInformation(in_);
      responses_[m]->Buffer().assign(response.begin() + (std::ptrdiff_t)(m * n), response.begin() + (std::ptrdiff_t)((m + 1) * n));
      indices_[m] = ScaleImageType::New();
      indices_[m]->CopyInformation(in_);
      indices_[m]->Buffer().assign(index.begin() + (std::ptrdiff_t)(m * n), index.begin() + (std::ptrdiff_t)((m + 1) * n));
    }
    dirty_ = false;
  }
  // measure m: its largest response over the scales, and the index of the scale (255: none)
  ResponseImageType *GetResponse(unsigned int m) { Update(); return at(responses_, m).GetPointer(); }
  ScaleImageType *GetScaleIndex(unsigned int m) { Update(); return at(indices_, m).GetPointer(); }

 private:
  template <typename V>
  static typename V::value_type &at(V &v, unsigned int m) {
    if (m >= v.size()) throw ExceptionObject("Measure index is out of range", "ScaleSelectImageFilter");
    return v[m];
  }
  const TImage *in_ = nullptr;
  const TMask *mask_ = nullptr;
  std::vector<float> scales_;
  std::vector<ife_scale_measure> measures_;
  std::vector<typename ResponseImageType::Pointer> responses_;
  std::vector<typename ScaleImageType::Pointer> indices_;
  bool dirty_ = true;
};

}  // namespace itk

#endif
