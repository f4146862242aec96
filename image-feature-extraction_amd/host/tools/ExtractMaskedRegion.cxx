// ExtractMaskedRegion -- a binary mask from a label map: `inside` where the label is one of the
// included values, `outside` elsewhere, on the device (ife_label_membership); the flags and
// messages of the reference's tools/ExtractMaskedRegion.cxx (-m -o -i... [-I 1] [-O 0]).  Pixels
// are unsigned short.
#include <cstdlib>
#include <iostream>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Host/RegionFilters.h"

const std::string VERSION("0.1");

int main(int argc, char *argv[]) {
  typedef unsigned short PixelType;
  TCLAP::CmdLine cmd("Extract part of a mask.", ' ', VERSION);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Path to output file", true, "", "path", cmd);
  TCLAP::MultiArg<PixelType> includeArg("i", "include", "Mask values to include", true, "PixelType", cmd);
  TCLAP::ValueArg<PixelType> insideArg("I", "inside", "Value to use for pixels that are included", false, 1,
                                       "PixelType", cmd);
  TCLAP::ValueArg<PixelType> outsideArg("O", "outside", "Value to use for pixels that are not included", false, 0,
                                        "PixelType", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string maskPath(maskArg.getValue()), outPath(outArg.getValue());
  const std::vector<PixelType> include(includeArg.getValue());

  typedef itk::Image<PixelType, 3> ImageType;
  itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
  reader->SetFileName(maskPath);
  typedef ife::LabelMembershipImageFilter<ImageType> FilterType;
  FilterType::Pointer filter = FilterType::New();
  filter->SetIncludeValues(include);
  filter->SetInsideValue(insideArg.getValue());
  filter->SetOutsideValue(outsideArg.getValue());
  itk::ImageFileWriter<ImageType>::Pointer writer = itk::ImageFileWriter<ImageType>::New();
  writer->SetFileName(outPath);
  try {
    reader->Update();
    filter->SetInput(reader->GetOutput());
    filter->Update();
    writer->SetInput(filter->GetOutput());
    writer->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to process." << std::endl
              << "Mask: " << maskPath << std::endl
              << "Out: " << outPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
