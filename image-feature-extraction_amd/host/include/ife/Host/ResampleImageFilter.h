// ResampleImageFilter.h -- itk::ResampleImageFilter, itk::TranslationTransform and the two
// interpolator tags as the reference's tools/Resample.cxx:83-99 wires them, on the device
// (ife_resample / ife_resample_f64; the arithmetic is defined in include/ife_hip.h).  Eager, no
// pipeline; direction cosines are ignored.  double, float, short, unsigned char and unsigned short
// pixels go to the device; any other type throws: there is no CPU path.
#ifndef IFE_HOST_RESAMPLEIMAGEFILTER_H
#define IFE_HOST_RESAMPLEIMAGEFILTER_H

#include <type_traits>

#include "ife/Host/Engine.h"

namespace itk {

// itk::Point - itk::Point = itk::Vector (Resample.cxx:90); both are three doubles here
inline Spacing3 operator-(const Spacing3 &a, const Spacing3 &b) {
  Spacing3 r;
  for (size_t d = 0; d < 3; ++d) r[d] = a[d] - b[d];
  return r;
}

// TranslationTransform<double, 3>: point + offset
template <typename TScalar, unsigned int VDim = 3>
class TranslationTransform {
  static_assert(VDim == 3 && std::is_same<TScalar, double>::value, "double, three dimensions");

 public:
  typedef TranslationTransform Self;
  typedef Spacing3 OutputVectorType;
  ifeNewMacro(Self);
  TranslationTransform() { for (size_t d = 0; d < 3; ++d) offset_[d] = 0.0; }
  void Translate(const OutputVectorType &t) {  // composes, as ITK's does
    for (size_t d = 0; d < 3; ++d) offset_[d] += t[d];
  }
  const OutputVectorType &GetOffset() const { return offset_; }

 private:
  OutputVectorType offset_;
};

// Interpolators are tags: they select IFE_INTERP_LINEAR / IFE_INTERP_NEAREST
template <typename TImage, typename TCoord = double>
class LinearInterpolateImageFunction {
 public:
  typedef LinearInterpolateImageFunction Self;
  ifeNewMacro(Self);
  static const int Interpolation = IFE_INTERP_LINEAR;
};
template <typename TImage, typename TCoord = double>
class NearestNeighborInterpolateImageFunction {
 public:
  typedef NearestNeighborInterpolateImageFunction Self;
  ifeNewMacro(Self);
  static const int Interpolation = IFE_INTERP_NEAREST;
};

namespace resample_detail {
// the device call of a pixel type; the primary template is every type without one
template <typename TIn, typename TOut>
struct Call {
  static int run(ife_ctx *, const TIn *, const ife_volume_desc *, const double *, const ife_volume_desc *,
                 const double *, const double *, int, double, TOut *) {
    throw ExceptionObject("pixel types double, float, short, unsigned char and unsigned short are resampled "
                          "(linear into float, nearest into the input's type; double into double)",
                          "ResampleImageFilter");
  }
};
template <>
struct Call<double, double> {
  static int run(ife_ctx *c, const double *s, const ife_volume_desc *sv, const double *so, const ife_volume_desc *dv,
                 const double *d_o, const double *t, int interp, double def, double *out) {
    return ife_resample_f64(c, s, sv, so, dv, d_o, t, interp, def, out, IFE_MEM_HOST);
  }
};
template <typename T> struct DType;
template <> struct DType<float> { static const int value = IFE_F32; };
template <> struct DType<short> { static const int value = IFE_I16; };
template <> struct DType<unsigned char> { static const int value = IFE_U8; };
template <> struct DType<unsigned short> { static const int value = IFE_U16; };
// linear writes float, nearest the input's type: the pair has to match the interpolation
template <typename TIn, typename TOut>
inline int typed(ife_ctx *c, const TIn *s, const ife_volume_desc *sv, const double *so, const ife_volume_desc *dv,
                 const double *d_o, const double *t, int interp, double def, TOut *out) {
  const bool fits = interp == IFE_INTERP_LINEAR ? std::is_same<TOut, float>::value : std::is_same<TOut, TIn>::value;
  if (!fits)
    throw ExceptionObject("linear interpolation writes float, nearest neighbour the input's pixel type",
                          "ResampleImageFilter");
  return ife_resample(c, s, DType<TIn>::value, sv, so, dv, d_o, t, interp, def, out, IFE_MEM_HOST);
}
#define IFE_RESAMPLE_CALL(TIn, TOut)                                                                        \
  template <>                                                                                               \
  struct Call<TIn, TOut> {                                                                                  \
    static int run(ife_ctx *c, const TIn *s, const ife_volume_desc *sv, const double *so,                   \
                   const ife_volume_desc *dv, const double *d_o, const double *t, int interp, double def,   \
                   TOut *out) {                                                                             \
      return typed<TIn, TOut>(c, s, sv, so, dv, d_o, t, interp, def, out);                                  \
    }                                                                                                       \
  }
IFE_RESAMPLE_CALL(float, float);
IFE_RESAMPLE_CALL(short, float);
IFE_RESAMPLE_CALL(short, short);
IFE_RESAMPLE_CALL(unsigned char, float);
IFE_RESAMPLE_CALL(unsigned char, unsigned char);
IFE_RESAMPLE_CALL(unsigned short, float);
IFE_RESAMPLE_CALL(unsigned short, unsigned short);
#undef IFE_RESAMPLE_CALL
}  // namespace resample_detail

template <typename TIn, typename TOut>
class ResampleImageFilter {
 public:
  typedef ResampleImageFilter Self;
  typedef TranslationTransform<double, 3> TransformType;
  ifeNewMacro(Self);
  void SetInput(const TIn *in) { in_ = in; dirty_ = true; }
  void SetTransform(const TransformType *t) { offset_ = t->GetOffset(); dirty_ = true; }
  void SetOutputOrigin(const Spacing3 &o) { origin_ = o; dirty_ = true; }
  void SetOutputSpacing(const Spacing3 &s) { spacing_ = s; dirty_ = true; }
  void SetSize(const Size3 &s) { size_ = s; dirty_ = true; }
  void SetDefaultPixelValue(typename TOut::PixelType v) { default_ = v; dirty_ = true; }
  template <typename TInterpolator>
  void SetInterpolator(const TInterpolator *) { interp_ = TInterpolator::Interpolation; dirty_ = true; }
  void Update() {
    if (!dirty_) return;
    if (!in_) throw ExceptionObject("Input is required", "ResampleImageFilter");
    ife::host::Engine &e = ife::host::Engine::Instance();
    if (out_.IsNull()) out_ = TOut::New();
    out_->SetRegions(size_);
    out_->SetSpacing(spacing_);
    out_->SetOrigin(origin_);
    out_->Allocate();
    const ife_volume_desc sv = ife::host::describe(*in_), dv = ife::host::describe(*out_);
    ife_ctx *ctx = e.ctx();
    e.check(resample_detail::Call<typename TIn::PixelType, typename TOut::PixelType>::run(
                ctx, in_->GetBufferPointer(), &sv, &in_->GetOrigin()[0], &dv, &origin_[0], &offset_[0], interp_,
                (double)default_, out_->GetBufferPointer()),
            "ResampleImageFilter");
    dirty_ = false;
  }
  void UpdateLargestPossibleRegion() { Update(); }
  TOut *GetOutput() { return out_.IsNull() ? (out_ = TOut::New()).GetPointer() : out_.GetPointer(); }

 private:
  const TIn *in_ = nullptr;
  Spacing3 offset_ = zero(), origin_ = zero(), spacing_;
  Size3 size_;
  typename TOut::PixelType default_ = 0;
  int interp_ = IFE_INTERP_LINEAR;
  bool dirty_ = true;
  typename TOut::Pointer out_;
  static Spacing3 zero() {
    Spacing3 z;
    z[0] = z[1] = z[2] = 0.0;
    return z;
  }
};

}  // namespace itk

#endif
