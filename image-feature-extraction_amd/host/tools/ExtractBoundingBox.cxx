// ExtractBoundingBox -- an image cut down to the bounding box of a mask's foreground, on the
// device (ife_mask_bounding_box, ife_extract_region); the flags and messages of the reference's
// tools/ExtractBoundingBox.cxx (-i -m -o).  The image is float, the mask is read as unsigned char
// and binarised by a clamp to [0, 1].  The output keeps the spacing and lies where the box lay:
// its origin and file geometry move by the box's index (DESIGN.md "Regions").
#include <cstdlib>
#include <iostream>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Host/LiteFilters.h"
#include "ife/Host/RegionFilters.h"

const std::string VERSION("0.1");

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Extract the bounding box of a mask from an image.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Path to output image", true, "", "path", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), maskPath(maskArg.getValue()), outPath(outArg.getValue());

  typedef itk::Image<float, 3> ImageType;
  typedef itk::Image<unsigned char, 3> MaskImageType;
  typedef MaskImageType::RegionType RegionType;

  itk::ImageFileReader<ImageType>::Pointer imageReader = itk::ImageFileReader<ImageType>::New();
  imageReader->SetFileName(imagePath);
  itk::ImageFileReader<MaskImageType>::Pointer maskReader = itk::ImageFileReader<MaskImageType>::New();
  maskReader->SetFileName(maskPath);
  try {
    imageReader->Update();
    maskReader->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Error reading images." << std::endl
              << "Image path:      " << imagePath << std::endl
              << "Mask path:       " << maskPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::ClampImageFilter<MaskImageType, MaskImageType> ClampFilterType;
  ClampFilterType::Pointer clampFilter = ClampFilterType::New();
  clampFilter->SetBounds(0, 1);
  clampFilter->SetInput(maskReader->GetOutput());
  typedef itk::ImageMaskSpatialObject<3> ImageMaskSpatialObject;
  ImageMaskSpatialObject::Pointer maskSO = ImageMaskSpatialObject::New();
  try {
    clampFilter->Update();
    maskSO->SetImage(clampFilter->GetOutput());
    maskSO->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Error calculating bounding box." << std::endl << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  const RegionType boundingBoxRegion = maskSO->GetAxisAlignedBoundingBoxRegion();

  typedef itk::ExtractImageFilter<ImageType, ImageType> ExtractImageFilterType;
  ExtractImageFilterType::Pointer extractFilter = ExtractImageFilterType::New();
  extractFilter->SetInput(imageReader->GetOutput());
  extractFilter->SetExtractionRegion(boundingBoxRegion);

  typedef itk::ImageFileWriter<ImageType> WriterType;
  WriterType::Pointer writer = WriterType::New();
  writer->SetFileName(outPath);
  try {  // a box that is not inside the image fails here, as it does in the reference's pipeline
    extractFilter->Update();
    writer->SetInput(extractFilter->GetOutput());
    writer->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to write image." << std::endl
              << "Out:             " << outPath << std::endl
              << "Bounding box:    " << boundingBoxRegion << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
