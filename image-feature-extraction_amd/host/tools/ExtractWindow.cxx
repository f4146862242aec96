// ExtractWindow -- an image onto a fine isotropic grid through a B-spline of order 0 to 5 with
// nearest-neighbour extrapolation, windowed to 8 bits, optionally masked; the flags of the
// reference's tools/ExtractWindow.cxx (-i -o [-m] [-w 1500] [-l -500] [-b 3]) and its target grid:
// size ceil(n * s / S) per axis, translation = the image's origin, output origin 0.  Ours:
// -S/--spacing (the reference fixes S = 0.25); volumes (the reference is 2-D: an axis of one voxel
// is absent here, it keeps its size and spacing, so a 2-D image behaves as it does there); and
// the mask is read from the mask's path (the reference opens the image's path for it, a slip).
#include <cmath>
#include <cstdlib>
#include <iostream>

#include "tclap/CmdLine.h"

#include "ife/Host/BSplineResampleImageFilter.h"
#include "ife/Host/ImageIO.h"

const std::string VERSION("0.1");

typedef itk::Image<double, 3> ImageType;
typedef itk::Image<unsigned char, 3> OutImageType;
typedef itk::BSplineResampleImageFilter<ImageType, ImageType> ResampleFilterType;

// `image` on the grid of spacing S through a spline of `order`, edges extended; what is said on
// stderr names the volume as `what`
static ResampleFilterType::Pointer resampleToSpacing(const ImageType *image, const itk::Spacing3 &translation,
                                                     double S, unsigned int order, const char *what) {
  const itk::Spacing3 spacing = image->GetSpacing();
  const itk::Size3 size = image->GetLargestPossibleRegion().GetSize();
  itk::Spacing3 newSpacing = spacing;
  itk::Size3 newSize = size;
  for (size_t i = 0; i < 3; ++i) {
    if (size[i] < 2) continue;
    newSpacing[i] = S;
    newSize[i] = (uint64_t)std::ceil(((double)size[i] * spacing[i]) / S);
  }
  typedef itk::TranslationTransform<double, 3> TransformType;
  const TransformType::Pointer transform = TransformType::New();
  transform->Translate(translation);
  typedef itk::BSplineInterpolateImageFunction<ImageType> InterpolatorType;
  InterpolatorType::Pointer interpolator = InterpolatorType::New();
  interpolator->SetSplineOrder(order);
  typedef itk::NearestNeighborExtrapolateImageFunction<ImageType, double> ExtrapolatorType;
  ExtrapolatorType::Pointer extrapolator = ExtrapolatorType::New();

  ResampleFilterType::Pointer filter = ResampleFilterType::New();
  filter->SetInput(image);
  filter->SetTransform(transform.GetPointer());
  filter->SetInterpolator(interpolator.GetPointer());
  filter->SetExtrapolator(extrapolator.GetPointer());
  filter->SetOutputSpacing(newSpacing);
  filter->SetSize(newSize);
  std::cerr << "Resampling " << what << "." << std::endl
            << "Origin:          " << image->GetOrigin() << std::endl
            << "Translation:     " << translation << std::endl
            << "OldSize:         " << size << std::endl
            << "Size:            " << newSize << std::endl
            << "Old spacing:     " << spacing << std::endl
            << "Spacing:         " << newSpacing << std::endl;
  filter->Update();
  return filter;
}

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Rescale intensity and convert to unsigned 8-bit.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Output path", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", false, "", "path", cmd);
  TCLAP::ValueArg<double> widthArg("w", "width", "Window width", false, 1500, "unsigned int", cmd);
  TCLAP::ValueArg<double> levelArg("l", "level", "Window level", false, -500, "int", cmd);
  TCLAP::ValueArg<unsigned int> splineOrderArg("b", "spline-order", "B-spline order for interpolation", false, 3,
                                               "[0,1,2,3,4,5]", cmd);
  TCLAP::ValueArg<double> spacingArg("S", "spacing", "Spacing of the output grid", false, 0.25, "double", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), outPath(outArg.getValue()), maskPath(maskArg.getValue());
  const double width(widthArg.getValue()), level(levelArg.getValue()), S(spacingArg.getValue());
  const unsigned int splineOrder(splineOrderArg.getValue());
  if (splineOrder > 5) {
    std::cerr << "Spline order must be <= 5" << std::endl;
    return EXIT_FAILURE;
  }
  if (!(S > 0.0) || !std::isfinite(S)) {
    std::cerr << "Spacing must be positive" << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::ImageFileReader<ImageType> ReaderType;
  ReaderType::Pointer imageReader = ReaderType::New(), maskReader = ReaderType::New();
  imageReader->SetFileName(imagePath);
  try {
    imageReader->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed reading image." << std::endl
              << "Path: " << imagePath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  if (!maskPath.empty()) {
    maskReader->SetFileName(maskPath);
    try {
      maskReader->Update();
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed reading mask." << std::endl
                << "Path: " << maskPath << std::endl
                << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
  }

  // both volumes move by the IMAGE's origin, as in the reference
  const itk::Spacing3 translation = imageReader->GetOutput()->GetOrigin();
  ResampleFilterType::Pointer resampleFilter, maskResampleFilter;
  try {
    resampleFilter = resampleToSpacing(imageReader->GetOutput(), translation, S, splineOrder, "image");
    if (!maskPath.empty())  // order 0: the mask stays binary
      maskResampleFilter = resampleToSpacing(maskReader->GetOutput(), translation, S, 0, "mask");
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to resample." << std::endl << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::IntensityWindowingImageFilter<ImageType, OutImageType> WindowFilterType;
  WindowFilterType::Pointer windowFilter = WindowFilterType::New();
  try {
    windowFilter->SetInput(resampleFilter->GetOutput());
    if (!maskPath.empty()) windowFilter->SetMaskImage(maskResampleFilter->GetOutput());
    windowFilter->SetWindowMinimum(level - width / 2);
    windowFilter->SetWindowMaximum(level + width / 2);
    windowFilter->SetOutputMinimum(0);
    windowFilter->SetOutputMaximum(255);
    windowFilter->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to window image." << std::endl
              << "Level:           " << level << std::endl
              << "Width:           " << width << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::ImageFileWriter<OutImageType> WriterType;
  WriterType::Pointer writer = WriterType::New();
  writer->SetFileName(outPath);
  writer->SetInput(windowFilter->GetOutput());
  try {
    writer->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to save image." << std::endl
              << "Out:             " << outPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
