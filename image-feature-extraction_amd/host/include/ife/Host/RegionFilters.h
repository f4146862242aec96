// RegionFilters.h -- the region filters the reference's preprocessing tools wire
// (tools/ExtractBoundingBox.cxx, ExtractSlices.cxx, PadImage.cxx, ExtractMaskedRegion.cxx), on the
// device: itk::ImageMaskSpatialObject<3> (ife_mask_bounding_box), itk::ExtractImageFilter,
// itk::ConstantPadImageFilter and itk::FlipImageFilter (all three ife_extract_region) and a
// membership filter of ours (ife_label_membership, the functor of ExtractMaskedRegion.cxx:62-67).
// Eager, no pipeline, through the Engine; there is no CPU path.  Direction cosines are ignored as
// everywhere in the mirror; the geometry of a cropped or padded output is csrc/region_plan.hpp's
// (DESIGN.md "Regions").
#ifndef IFE_HOST_REGIONFILTERS_H
#define IFE_HOST_REGIONFILTERS_H

#include <array>
#include <sstream>
#include <vector>

#include "ife/Host/Engine.h"
#include "region_plan.hpp"

namespace ife {
namespace host {

// what ife_mask_bounding_box reads
template <typename T> struct BoxDType;
template <> struct BoxDType<unsigned char> { static const int value = IFE_U8; };
template <> struct BoxDType<unsigned short> { static const int value = IFE_U16; };
template <> struct BoxDType<short> { static const int value = IFE_I16; };
template <> struct BoxDType<float> { static const int value = IFE_F32; };

// The tightest box around the foreground of `mask` and the number of foreground voxels; an empty
// mask gives an empty region and 0.
template <typename TMask>
inline int64_t mask_bounding_box(const TMask &mask, itk::Region3 &region, const char *where) {
  Engine &e = Engine::Instance();
  const ife_volume_desc d = describe(mask);
  int64_t box[6], count = 0;
  ife_ctx *ctx = e.ctx();
  e.check(ife_mask_bounding_box(ctx, mask.GetBufferPointer(), BoxDType<typename TMask::PixelType>::value, &d, box,
                                &count, IFE_MEM_HOST),
          where);
  for (size_t a = 0; a < 3; ++a) {
    region.index[a] = box[a];
    region.size[a] = (uint64_t)box[3 + a];
  }
  return count;
}

// `out` takes the geometry of the box at `index` of `in`: the spacing stays, the origin moves to
// origin + index o spacing; NIfTI geometry moves its sform offsets by the sform's columns and its
// qoffset by the quaternion's rotation, a MetaImage Offset by its TransformMatrix.
inline void shift_geometry(const itk::ImageBase3 &in, const itk::Index3 &index, itk::ImageBase3 &out) {
  const int64_t idx[3] = {index[0], index[1], index[2]};
  const double spacing[3] = {in.GetSpacing()[0], in.GetSpacing()[1], in.GetSpacing()[2]};
  const double origin[3] = {in.GetOrigin()[0], in.GetOrigin()[1], in.GetOrigin()[2]};
  double moved[3];
  region_shift_origin(origin, spacing, idx, moved);
  itk::FileGeometry g = in.GetFileGeometry();
  if (g.has_nifti) {
    region_shift_srow(g.srow, idx);
    region_shift_qoffset(g.quatern, g.qfac, spacing, idx, g.qoffset);
  }
  if (g.has_mhd && !g.mhd_transform.empty()) {
    std::istringstream is(g.mhd_transform);
    double m[9];
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && (is >> m[i]);
    if (ok) {
      for (int a = 0; a < 3; ++a) moved[a] = origin[a];
      region_shift_mhd_offset(m, spacing, idx, moved);
    }
  }
  itk::Spacing3 o;
  for (size_t a = 0; a < 3; ++a) o[a] = moved[a];
  out.SetSpacing(in.GetSpacing());
  out.SetOrigin(o);
  out.SetFileGeometry(g);
}

// a buffer on the Engine's device, freed with its owner (ife_device_alloc)
class DeviceBuffer {
 public:
  DeviceBuffer() {}
  ~DeviceBuffer() { reset(); }
  void reset() {
    if (p_) ife_device_free(Engine::Instance().ctx(), p_);
    p_ = nullptr;
  }
  void upload(const void *src, size_t bytes, const char *where) {
    Engine &e = Engine::Instance();
    reset();
    ife_ctx *ctx = e.ctx();
    e.check(ife_device_alloc(ctx, bytes, &p_), where);
    e.check(ife_device_upload(ctx, p_, src, bytes), where);
  }
  const void *get() const { return p_; }

 private:
  DeviceBuffer(const DeviceBuffer &);
  DeviceBuffer &operator=(const DeviceBuffer &);
  void *p_ = nullptr;
};

}  // namespace host
}  // namespace ife

namespace itk {

template <typename T, unsigned int N>
struct FixedArray {
  std::array<T, N> v;
  T &operator[](size_t i) { return v[i]; }
  const T &operator[](size_t i) const { return v[i]; }
};

// itk::ImageMaskSpatialObject<3> as ExtractBoundingBox.cxx:95-107 uses it.  Update() throws on a
// mask without foreground (the tool's "Error calculating bounding box.").
template <unsigned int VDim = 3>
class ImageMaskSpatialObject {
  static_assert(VDim == 3, "three dimensions");

 public:
  typedef ImageMaskSpatialObject Self;
  typedef Image<unsigned char, 3> ImageType;
  typedef Region3 RegionType;
  ifeNewMacro(Self);
  void SetImage(const ImageType *image) { image_ = image; }
  void Update() {
    if (!image_) throw ExceptionObject("Image is required", "ImageMaskSpatialObject");
    count_ = ife::host::mask_bounding_box(*image_, region_, "ImageMaskSpatialObject");
    if (count_ == 0) throw ExceptionObject("the mask has no foreground", "ImageMaskSpatialObject");
  }
  RegionType GetAxisAlignedBoundingBoxRegion() const { return region_; }
  int64_t GetNumberOfForegroundPixels() const { return count_; }

 private:
  const ImageType *image_ = nullptr;
  Region3 region_;
  int64_t count_ = 0;
};

namespace region_detail {
// one ife_extract_region of a host or device source into a host image
template <typename TPixel>
inline void extract(const void *src, int src_mem, const ImageBase3 &src_info, const Index3 &index, const Size3 &size,
                    int flip, const TPixel *pad, TPixel *dst, const char *where) {
  ife::host::Engine &e = ife::host::Engine::Instance();
  const ife_volume_desc d = ife::host::describe(src_info);
  const int64_t region[6] = {index[0], index[1], index[2], (int64_t)size[0], (int64_t)size[1], (int64_t)size[2]};
  ife_ctx *ctx = e.ctx();
  e.check(ife_extract_region(ctx, src, (int)sizeof(TPixel), &d, region, flip, pad, dst, src_mem, IFE_MEM_HOST), where);
}
}  // namespace region_detail

// itk::ExtractImageFilter / RegionOfInterestImageFilter: the extraction region must lie inside
// the input.  A size of 0 along an axis collapses it (ExtractSlices.cxx:238-245); the output then
// is the volume (a, b, 1) of the two remaining axes in order, with their spacings and the origin
// of the slice's start index, and carries no file geometry (SetDirectionCollapseToIdentity).
// Ours: SetFlipAxes folds the itk::FlipImageFilter behind the extraction into the same gather
// (axes of the INPUT), and SetDeviceResident(true) uploads the input once and serves every later
// Update from the device copy until SetInput is called again.
template <typename TIn, typename TOut>
class ExtractImageFilter {
 public:
  typedef ExtractImageFilter Self;
  typedef typename TIn::PixelType PixelType;
  ifeNewMacro(Self);
  void SetInput(const TIn *in) { in_ = in; resident_.reset(); uploaded_ = false; }
  void SetExtractionRegion(const Region3 &r) { region_ = r; }
  void SetDirectionCollapseToIdentity() {}
  void SetFlipAxes(const FixedArray<bool, 3> &f) { flip_ = (f[0] ? 1 : 0) | (f[1] ? 2 : 0) | (f[2] ? 4 : 0); }
  void SetDeviceResident(bool on) { device_ = on; }
  void Update() {
    static_assert(std::is_same<typename TIn::PixelType, typename TOut::PixelType>::value, "bits are copied");
    if (!in_) throw ExceptionObject("Input is required", "ExtractImageFilter");
    Size3 size = region_.size;
    int collapsed = -1;
    for (size_t a = 0; a < 3; ++a)
      if (size[a] == 0) { size[a] = 1; collapsed = (int)a; }
    if (!in_->GetLargestPossibleRegion().IsInside(Region3(region_.index, size))) {
      std::ostringstream os;
      os << "Requested region is (at least partially) outside the largest possible region: " << region_
         << " of " << in_->GetLargestPossibleRegion();
      throw ExceptionObject(os.str(), "ExtractImageFilter");
    }
    const void *src = in_->GetBufferPointer();
    int src_mem = IFE_MEM_HOST;
    if (device_) {
      if (!uploaded_) {
        resident_.upload(src, (size_t)in_->GetLargestPossibleRegion().GetNumberOfPixels() * sizeof(PixelType),
                         "ExtractImageFilter");
        uploaded_ = true;
      }
      src = resident_.get();
      src_mem = IFE_MEM_DEVICE;
    }
    out_ = TOut::New();
    if (collapsed < 0) {
      out_->SetRegions(size);
      ife::host::shift_geometry(*in_, region_.index, *out_);
    } else {
      Size3 s2;
      Spacing3 sp, og;
      size_t k = 0;
      for (size_t a = 0; a < 3; ++a) {
        if ((int)a == collapsed) continue;
        s2[k] = size[a];
        sp[k] = in_->GetSpacing()[a];
        og[k] = in_->GetOrigin()[a] + (double)region_.index[a] * in_->GetSpacing()[a];
        ++k;
      }
      s2[2] = 1; sp[2] = 1.0; og[2] = 0.0;
      out_->SetRegions(s2);
      out_->SetSpacing(sp);
      out_->SetOrigin(og);
    }
    out_->Allocate();
    region_detail::extract<PixelType>(src, src_mem, *in_, region_.index, size, flip_, nullptr,
                                      out_->GetBufferPointer(), "ExtractImageFilter");
  }
  TOut *GetOutput() { return out_.GetPointer(); }

 private:
  const TIn *in_ = nullptr;
  Region3 region_;
  int flip_ = 0;
  bool device_ = false, uploaded_ = false;
  ife::host::DeviceBuffer resident_;
  typename TOut::Pointer out_;
};

// itk::ConstantPadImageFilter: lower and upper pad per axis, the constant elsewhere; the output's
// origin moves by -lower (index -lower, size n + lower + upper of ife_extract_region).
template <typename TIn, typename TOut>
class ConstantPadImageFilter {
 public:
  typedef ConstantPadImageFilter Self;
  typedef typename TIn::PixelType PixelType;
  ifeNewMacro(Self);
  void SetInput(const TIn *in) { in_ = in; }
  void SetConstant(PixelType v) { constant_ = v; }
  void SetPadLowerBound(const Size3 &s) { lower_ = s; }
  void SetPadUpperBound(const Size3 &s) { upper_ = s; }
  void Update() {
    static_assert(std::is_same<typename TIn::PixelType, typename TOut::PixelType>::value, "bits are copied");
    if (!in_) throw ExceptionObject("Input is required", "ConstantPadImageFilter");
    const Size3 &n = in_->GetLargestPossibleRegion().GetSize();
    Index3 index;
    Size3 size;
    for (size_t a = 0; a < 3; ++a) {
      // what an unsigned subtraction that wrapped leaves (PadImage.cxx:65) cannot be allocated
      if (lower_[a] > ((uint64_t)1 << 40) || upper_[a] > ((uint64_t)1 << 40))
        throw ExceptionObject("the pad bounds are too large to allocate the output", "ConstantPadImageFilter");
      index[a] = -(int64_t)lower_[a];
      size[a] = n[a] + lower_[a] + upper_[a];
    }
    out_ = TOut::New();
    out_->SetRegions(size);
    ife::host::shift_geometry(*in_, index, *out_);
    out_->Allocate();
    region_detail::extract<PixelType>(in_->GetBufferPointer(), IFE_MEM_HOST, *in_, index, size, 0, &constant_,
                                      out_->GetBufferPointer(), "ConstantPadImageFilter");
  }
  TOut *GetOutput() { return out_.GetPointer(); }

 private:
  const TIn *in_ = nullptr;
  PixelType constant_ = PixelType();
  Size3 lower_, upper_;
  typename TOut::Pointer out_;
};

// itk::FlipImageFilter: the voxels mirrored along the chosen axes; the geometry is the input's
// (ours: ITK also mirrors the origin, which the mirror, without directions, does not express).
template <typename TImage>
class FlipImageFilter {
 public:
  typedef FlipImageFilter Self;
  typedef FixedArray<bool, 3> FlipAxesArrayType;
  ifeNewMacro(Self);
  void SetInput(const TImage *in) { in_ = in; }
  void SetFlipAxes(const FlipAxesArrayType &f) { flip_ = (f[0] ? 1 : 0) | (f[1] ? 2 : 0) | (f[2] ? 4 : 0); }
  void Update() {
    if (!in_) throw ExceptionObject("Input is required", "FlipImageFilter");
    out_ = TImage::New();
    out_->CopyInformation(in_);
    out_->Allocate();
    region_detail::extract<typename TImage::PixelType>(in_->GetBufferPointer(), IFE_MEM_HOST, *in_, Index3(),
                                                       in_->GetLargestPossibleRegion().GetSize(), flip_, nullptr,
                                                       out_->GetBufferPointer(), "FlipImageFilter");
  }
  TImage *GetOutput() { return out_.GetPointer(); }

 private:
  const TImage *in_ = nullptr;
  int flip_ = 0;
  typename TImage::Pointer out_;
};

}  // namespace itk

namespace ife {

// Ours: inside where the pixel occurs in the set, outside elsewhere (the UnaryFunctorImageFilter
// with the MembershipFunctor of ExtractMaskedRegion.cxx:157-163).  unsigned char and unsigned
// short pixels.
template <typename TImage>
class LabelMembershipImageFilter {
 public:
  typedef LabelMembershipImageFilter Self;
  typedef typename TImage::PixelType PixelType;
  ifeNewMacro(Self);
  void SetInput(const TImage *in) { in_ = in; }
  void SetIncludeValues(const std::vector<PixelType> &v) { include_.assign(v.begin(), v.end()); }
  void SetInsideValue(PixelType v) { inside_ = v; }
  void SetOutsideValue(PixelType v) { outside_ = v; }
  void Update() {
    if (!in_) throw itk::ExceptionObject("Input is required", "LabelMembershipImageFilter");
    host::Engine &e = host::Engine::Instance();
    out_ = TImage::New();
    out_->CopyInformation(in_);
    out_->Allocate();
    ife_ctx *ctx = e.ctx();
    e.check(ife_label_membership(ctx, in_->GetBufferPointer(), host::MaskDType<PixelType>::value,
                                 (int64_t)in_->GetLargestPossibleRegion().GetNumberOfPixels(),
                                 include_.empty() ? nullptr : include_.data(), (int)include_.size(), (int)inside_,
                                 (int)outside_, out_->GetBufferPointer(), IFE_MEM_HOST),
            "LabelMembershipImageFilter");
  }
  TImage *GetOutput() { return out_.GetPointer(); }

 private:
  const TImage *in_ = nullptr;
  std::vector<int> include_;
  PixelType inside_ = 1, outside_ = 0;
  typename TImage::Pointer out_;
};

}  // namespace ife

#endif
