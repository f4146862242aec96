// BSplineResampleImageFilter.h -- itk::ResampleImageFilter with an
// itk::BSplineInterpolateImageFunction (orders 0 to 5) and, optionally, an
// itk::NearestNeighborExtrapolateImageFunction, as the reference's tools/ExtractWindow.cxx wires
// them, and itk::IntensityWindowingImageFilter to unsigned char with a mask; all on the device
// (ife_resample_bspline*, ife_window_u8; the arithmetic is defined in include/ife_hip.h).  Eager,
// no pipeline; direction cosines are ignored.  double pixels come back as double; float, short,
// unsigned char and unsigned short come back as float; any other pair throws or does not compile:
// there is no CPU path.
#ifndef IFE_HOST_BSPLINERESAMPLEIMAGEFILTER_H
#define IFE_HOST_BSPLINERESAMPLEIMAGEFILTER_H

#include "ife/Host/ResampleImageFilter.h"

namespace itk {

// the interpolator carries the order; nothing else of it is used
template <typename TImage, typename TCoord = double, typename TCoefficient = double>
class BSplineInterpolateImageFunction {
 public:
  typedef BSplineInterpolateImageFunction Self;
  ifeNewMacro(Self);
  void SetSplineOrder(unsigned int order) { order_ = order; }
  unsigned int GetSplineOrder() const { return order_; }

 private:
  unsigned int order_ = 3;
};

// a tag: outside voxels take the nearest source voxel instead of the default value
template <typename TImage, typename TCoord = double>
class NearestNeighborExtrapolateImageFunction {
 public:
  typedef NearestNeighborExtrapolateImageFunction Self;
  ifeNewMacro(Self);
};

namespace bspline_detail {
template <typename TIn, typename TOut>
struct Call {
  static int run(ife_ctx *, const TIn *, const ife_volume_desc *, const double *, const ife_volume_desc *,
                 const double *, const double *, int, int, double, TOut *) {
    throw ExceptionObject("B-spline resampling takes double into double, and float, short, unsigned char and "
                          "unsigned short into float",
                          "BSplineResampleImageFilter");
  }
};
template <>
struct Call<double, double> {
  static int run(ife_ctx *c, const double *s, const ife_volume_desc *sv, const double *so, const ife_volume_desc *dv,
                 const double *d_o, const double *t, int order, int extrapolate, double def, double *out) {
    return ife_resample_bspline_f64(c, s, sv, so, dv, d_o, t, order, extrapolate, def, out, IFE_MEM_HOST);
  }
};
template <typename TIn>
struct Call<TIn, float> {
  static int run(ife_ctx *c, const TIn *s, const ife_volume_desc *sv, const double *so, const ife_volume_desc *dv,
                 const double *d_o, const double *t, int order, int extrapolate, double def, float *out) {
    return ife_resample_bspline(c, s, resample_detail::DType<TIn>::value, sv, so, dv, d_o, t, order, extrapolate, def,
                                out, IFE_MEM_HOST);
  }
};
}  // namespace bspline_detail

template <typename TIn, typename TOut>
class BSplineResampleImageFilter {
 public:
  typedef BSplineResampleImageFilter Self;
  typedef TranslationTransform<double, 3> TransformType;
  ifeNewMacro(Self);
  void SetInput(const TIn *in) { in_ = in; dirty_ = true; }
  void SetTransform(const TransformType *t) { offset_ = t->GetOffset(); dirty_ = true; }
  void SetOutputOrigin(const Spacing3 &o) { origin_ = o; dirty_ = true; }
  void SetOutputSpacing(const Spacing3 &s) { spacing_ = s; dirty_ = true; }
  void SetSize(const Size3 &s) { size_ = s; dirty_ = true; }
  void SetDefaultPixelValue(typename TOut::PixelType v) { default_ = v; dirty_ = true; }
  void SetSplineOrder(unsigned int order) { order_ = order; dirty_ = true; }
  template <typename TImage, typename TCoord, typename TCoefficient>
  void SetInterpolator(const BSplineInterpolateImageFunction<TImage, TCoord, TCoefficient> *f) {
    SetSplineOrder(f->GetSplineOrder());
  }
  template <typename TImage, typename TCoord>
  void SetInterpolator(const NearestNeighborInterpolateImageFunction<TImage, TCoord> *) {
    SetSplineOrder(0);  // the spline of order 0 is the nearest neighbour
  }
  template <typename TImage, typename TCoord>
  void SetExtrapolator(const NearestNeighborExtrapolateImageFunction<TImage, TCoord> *f) {
    extrapolate_ = f != nullptr;
    dirty_ = true;
  }
  void Update() {
    if (!dirty_) return;
    if (!in_) throw ExceptionObject("Input is required", "BSplineResampleImageFilter");
    ife::host::Engine &e = ife::host::Engine::Instance();
    if (out_.IsNull()) out_ = TOut::New();
    out_->SetRegions(size_);
    out_->SetSpacing(spacing_);
    out_->SetOrigin(origin_);
    out_->Allocate();
    const ife_volume_desc sv = ife::host::describe(*in_), dv = ife::host::describe(*out_);
    ife_ctx *ctx = e.ctx();
    e.check(bspline_detail::Call<typename TIn::PixelType, typename TOut::PixelType>::run(
                ctx, in_->GetBufferPointer(), &sv, &in_->GetOrigin()[0], &dv, &origin_[0], &offset_[0], (int)order_,
                extrapolate_ ? 1 : 0, (double)default_, out_->GetBufferPointer()),
            "BSplineResampleImageFilter");
    dirty_ = false;
  }
  void UpdateLargestPossibleRegion() { Update(); }
  TOut *GetOutput() { return out_.IsNull() ? (out_ = TOut::New()).GetPointer() : out_.GetPointer(); }

 private:
  const TIn *in_ = nullptr;
  Spacing3 offset_ = zero(), origin_ = zero(), spacing_;
  Size3 size_;
  typename TOut::PixelType default_ = 0;
  unsigned int order_ = 3;
  bool extrapolate_ = false, dirty_ = true;
  typename TOut::Pointer out_;
  static Spacing3 zero() {
    Spacing3 z;
    z[0] = z[1] = z[2] = 0.0;
    return z;
  }
};

// double in, unsigned char out; SetMaskImage (ours) folds itk::MaskImageFilter with outside value
// 0 into the same pass: where the mask is 0 the output is 0
template <typename TIn, typename TOut>
class IntensityWindowingImageFilter {
  static_assert(std::is_same<typename TIn::PixelType, double>::value &&
                    std::is_same<typename TOut::PixelType, unsigned char>::value,
                "double pixels windowed to unsigned char");

 public:
  typedef IntensityWindowingImageFilter Self;
  ifeNewMacro(Self);
  void SetInput(const TIn *in) { in_ = in; }
  void SetMaskImage(const TIn *mask) { mask_ = mask; }
  void SetWindowMinimum(double v) { wmin_ = v; }
  void SetWindowMaximum(double v) { wmax_ = v; }
  void SetOutputMinimum(unsigned char v) { omin_ = v; }
  void SetOutputMaximum(unsigned char v) { omax_ = v; }
  void Update() {
    if (!in_) throw ExceptionObject("Input is required", "IntensityWindowingImageFilter");
    if (mask_) ife::host::same_size(*in_, *mask_, "IntensityWindowingImageFilter");
    ife::host::Engine &e = ife::host::Engine::Instance();
    if (out_.IsNull()) out_ = TOut::New();
    out_->CopyInformation(in_);
    out_->Allocate();
    e.check(ife_window_u8(e.ctx(), in_->GetBufferPointer(), mask_ ? mask_->GetBufferPointer() : nullptr,
                          (int64_t)in_->GetLargestPossibleRegion().GetNumberOfPixels(), wmin_, wmax_, omin_, omax_,
                          out_->GetBufferPointer(), IFE_MEM_HOST),
            "IntensityWindowingImageFilter");
  }
  TOut *GetOutput() { return out_.IsNull() ? (out_ = TOut::New()).GetPointer() : out_.GetPointer(); }

 private:
  const TIn *in_ = nullptr, *mask_ = nullptr;
  double wmin_ = 0.0, wmax_ = 255.0;
  unsigned char omin_ = 0, omax_ = 255;
  typename TOut::Pointer out_;
};

}  // namespace itk

#endif
