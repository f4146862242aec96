// PadImage -- an image padded with a constant to a given size in x and y, the image centred
// (the odd voxel goes to the upper side), on the device (ife_extract_region); the flags and
// messages of the reference's tools/PadImage.cxx (-i -o -x -y [-p 0]).  Pixels are short.  The
// reference is 2-D; here a slice arrives as a volume with nz = 1, and a deeper volume is padded
// plane by plane: z is untouched.  A target below the image's size fails with "Error padding
// image." (the reference's unsigned subtraction wraps there and ITK throws).
#include <cstdlib>
#include <iostream>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Host/RegionFilters.h"

const std::string VERSION = "0.1";

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Pad image to a given size with a constant value", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Out path", true, "", "path", cmd);
  TCLAP::ValueArg<unsigned int> sizeXArg("x", "size-x", "size in x axis", true, 0, "unsigned int", cmd);
  TCLAP::ValueArg<unsigned int> sizeYArg("y", "size-y", "size in y axis", true, 0, "unsigned int", cmd);
  TCLAP::ValueArg<short> padArg("p", "pad-value", "Value to use for padding", false, 0, "short", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << "for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), outPath(outArg.getValue());
  const unsigned int target[2] = {sizeXArg.getValue(), sizeYArg.getValue()};

  typedef short PixelType;
  typedef itk::Image<PixelType, 3> ImageType;
  itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
  reader->SetFileName(imagePath);
  try {
    reader->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Error reading image." << std::endl
              << "Image           : " << imagePath << std::endl
              << "ExceptionObject : " << e << std::endl;
    return EXIT_FAILURE;
  }

  typedef itk::ConstantPadImageFilter<ImageType, ImageType> PadFilterType;
  PadFilterType::Pointer padFilter = PadFilterType::New();
  padFilter->SetInput(reader->GetOutput());
  padFilter->SetConstant(padArg.getValue());
  const ImageType::SizeType size = reader->GetOutput()->GetLargestPossibleRegion().GetSize();
  ImageType::SizeType padSize, lowerBound, upperBound;   // z: 0
  for (size_t i = 0; i < 2; ++i) {
    padSize[i] = (uint64_t)target[i] - size[i];          // wraps where the target is too small
    lowerBound[i] = padSize[i] / 2;
    upperBound[i] = lowerBound[i] + padSize[i] % 2;
  }
  padFilter->SetPadLowerBound(lowerBound);
  padFilter->SetPadUpperBound(upperBound);
  try {
    padFilter->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Error padding image." << std::endl
              << "Image           : " << imagePath << std::endl
              << "Size            : " << size << std::endl
              << "PadSize         : " << padSize << std::endl
              << "LowerBound      : " << lowerBound << std::endl
              << "UpperBound      : " << upperBound << std::endl
              << "ExceptionObject : " << e << std::endl;
    return EXIT_FAILURE;
  }

  itk::ImageFileWriter<ImageType>::Pointer writer = itk::ImageFileWriter<ImageType>::New();
  writer->SetInput(padFilter->GetOutput());
  writer->SetFileName(outPath);
  try {
    writer->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Error writing image." << std::endl
              << "Image           : " << imagePath << std::endl
              << "OutPath         : " << outPath << std::endl
              << "ExceptionObject : " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
