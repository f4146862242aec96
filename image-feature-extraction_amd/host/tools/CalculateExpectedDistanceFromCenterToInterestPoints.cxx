// CalculateExpectedDistanceFromCenterToInterestPoints -- mean over the mask of (signed distance
// to the mask's border, inside positive) * probability; flags and output of the reference's
// tools/CalculateExpectedDistanceFromCenterToInterestPoints.cxx (:18-36: -p -m; :79: the value
// on one line).
#include <iostream>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Statistics/ExpectedDistanceFromCenterToInterestPoint.h"

const std::string VERSION("0.1");

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Expected distance from center to interest points.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("p", "prob-image",
                                        "Path to probability image, expected to hold values in [0,1].", true, "",
                                        "path", cmd);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", true, "", "path", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), maskPath(maskArg.getValue());
  typedef itk::Image<double, 3> ImageType;
  typedef itk::Image<unsigned int, 3> MaskType;
  try {
    itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
    reader->SetFileName(imagePath);
    itk::ImageFileReader<MaskType>::Pointer maskReader = itk::ImageFileReader<MaskType>::New();
    maskReader->SetFileName(maskPath);
    reader->Update();
    maskReader->Update();
    const double ed =
        expectedDistanceFromCenterToInterestPoint<MaskType, ImageType>(maskReader->GetOutput(), reader->GetOutput());
    std::cout << ed << std::endl;
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to process." << std::endl
              << "Image: " << imagePath << std::endl
              << "Mask: " << maskPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
