// Resample -- a source image onto the grid of a target image, double pixels, linear, default 0;
// flags, printed lines and error messages of the reference's tools/Resample.cxx (:27-34: -s -t -o).
// The translation is source origin - target origin (:90), so the origins cancel in
// c = ((O_t + i s_t) + (O_s - O_t) - O_s) / s_s: the tool aligns the two index-zero voxels, as the
// reference does.  IFE_RESAMPLE_NEAREST=1 selects nearest neighbour (the reference has no flag).
// -b/--spline-order (ours, optional) interpolates with a B-spline of that order, 0 to 5, instead;
// without it the tool does what it did before the flag existed.
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Host/BSplineResampleImageFilter.h"
#include "ife/Host/ResampleImageFilter.h"

const std::string VERSION("0.1");

template <typename TImage>
static void printInformation(const TImage *image) {
  std::cout << "Origin " << image->GetOrigin() << std::endl
            << "Spacing " << image->GetSpacing() << std::endl
            << "Direction " << image->GetDirection() << std::endl
            << "Size " << image->GetLargestPossibleRegion().GetSize() << std::endl;
}

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd(
      "Resample a <source> image to match the pixel spacing of a <target> image. "
      "It is assumed that the images have the same coordinate system and are perfectly registered. "
      "This is intended for resampling a segmentation mask from one reconstruction thickness to another "
      "reconstruction thickness.",
      ' ', VERSION);
  TCLAP::ValueArg<std::string> sourceArg("s", "source", "Path to source image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> targetArg("t", "target", "Path to target image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Path to output image", true, "", "path", cmd);
  TCLAP::ValueArg<unsigned int> splineOrderArg("b", "spline-order", "B-spline order for interpolation (default: linear)",
                                               false, 3, "[0,1,2,3,4,5]", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string sourcePath(sourceArg.getValue()), targetPath(targetArg.getValue()), outPath(outArg.getValue());
  if (splineOrderArg.isSet() && splineOrderArg.getValue() > 5) {
    std::cerr << "Spline order must be <= 5" << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::Image<double, 3> ImageType;
  typedef itk::ImageFileReader<ImageType> ReaderType;
  ReaderType::Pointer sourceReader = ReaderType::New();
  ReaderType::Pointer targetReader = ReaderType::New();
  sourceReader->SetFileName(sourcePath);
  targetReader->SetFileName(targetPath);
  try {
    sourceReader->Update();
    targetReader->Update();
    std::cout << "== Source ==" << std::endl;
    printInformation(sourceReader->GetOutput());
    std::cout << "== Target ==" << std::endl;
    printInformation(targetReader->GetOutput());
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to read images" << std::endl
              << "Source image path: " << sourcePath << std::endl
              << "Target image path: " << targetPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::ImageFileWriter<ImageType> WriterType;
  WriterType::Pointer writer = WriterType::New();
  if (splineOrderArg.isSet()) {  // the same grid and translation through a B-spline, default 0
    typedef itk::BSplineResampleImageFilter<ImageType, ImageType> BSplineFilterType;
    BSplineFilterType::Pointer splineFilter = BSplineFilterType::New();
    try {
      typedef itk::TranslationTransform<double, 3> TransformType;
      const TransformType::Pointer transform = TransformType::New();
      TransformType::OutputVectorType translation;
      translation = sourceReader->GetOutput()->GetOrigin() - targetReader->GetOutput()->GetOrigin();
      std::cout << "Translation: " << translation << std::endl;
      transform->Translate(translation);
      splineFilter->SetInput(sourceReader->GetOutput());
      splineFilter->SetTransform(transform.GetPointer());
      splineFilter->SetSplineOrder(splineOrderArg.getValue());
      splineFilter->SetOutputOrigin(targetReader->GetOutput()->GetOrigin());
      splineFilter->SetOutputSpacing(targetReader->GetOutput()->GetSpacing());
      splineFilter->SetSize(targetReader->GetOutput()->GetLargestPossibleRegion().GetSize());
      splineFilter->Update();
      splineFilter->GetOutput()->CopyInformation(targetReader->GetOutput());
      std::cout << "Source image information after resampling" << std::endl;
      printInformation(splineFilter->GetOutput());
      writer->SetFileName(outPath);
      writer->SetInput(splineFilter->GetOutput());
      writer->Update();
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed to process." << std::endl
                << "Source image: " << sourcePath << std::endl
                << "Target image: " << targetPath << std::endl
                << "Out path: " << outPath << std::endl
                << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
  }

  typedef itk::ResampleImageFilter<ImageType, ImageType> ResampleFilterType;
  ResampleFilterType::Pointer resampleFilter = ResampleFilterType::New();
  try {
    resampleFilter->SetInput(sourceReader->GetOutput());

    typedef itk::TranslationTransform<double, 3> TransformType;
    const TransformType::Pointer transform = TransformType::New();
    TransformType::OutputVectorType translation;
    translation = sourceReader->GetOutput()->GetOrigin() - targetReader->GetOutput()->GetOrigin();
    std::cout << "Translation: " << translation << std::endl;
    transform->Translate(translation);
    resampleFilter->SetTransform(transform);

    const char *nearest = std::getenv("IFE_RESAMPLE_NEAREST");
    if (nearest && nearest[0] && std::strcmp(nearest, "0") != 0)
      resampleFilter->SetInterpolator(itk::NearestNeighborInterpolateImageFunction<ImageType>::New().GetPointer());

    resampleFilter->SetOutputOrigin(targetReader->GetOutput()->GetOrigin());
    resampleFilter->SetOutputSpacing(targetReader->GetOutput()->GetSpacing());
    resampleFilter->SetSize(targetReader->GetOutput()->GetLargestPossibleRegion().GetSize());
    resampleFilter->UpdateLargestPossibleRegion();
    // the file geometry of the target (qform / sform, MetaImage transform) goes with its grid
    resampleFilter->GetOutput()->CopyInformation(targetReader->GetOutput());

    writer->SetFileName(outPath);
    writer->SetInput(resampleFilter->GetOutput());
    resampleFilter->Update();
    std::cout << "Source image information after resampling" << std::endl;
    printInformation(resampleFilter->GetOutput());
    writer->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to process." << std::endl
              << "Source image: " << sourcePath << std::endl
              << "Target image: " << targetPath << std::endl
              << "Out path: " << outPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
