// GenerateROIs -- boxes drawn at random such that the centre of every box is a voxel of the mask
// with the requested value and the box lies inside the image.  Flags, defaults, output file and
// messages of the reference's tools/GenerateROIs.cxx (-m -o [-n 50] [-x 53] [-y 53] [-z 41]
// [-M 1]; one line "[x, y, z][sx, sy, sz]" per box; "Failed to generate ROIs." where no voxel
// admits a box, which the reference answers by drawing forever).  The draws are the device's
// (ife_random_rois, include/ife_hip.h states them); IFE_SEED fixes the seed, unset it comes from
// std::random_device.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/ROI/DeviceSampling.h"

const std::string VERSION("0.2");

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Generate 3D ROIs.", ' ', VERSION);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outFileArg("o", "outfile", "Path to output file", true, "", "path", cmd);
  TCLAP::ValueArg<unsigned int> numROIsArg("n", "num-rois", "Number of ROIs to sample", false, 50, "unsigned int", cmd);
  TCLAP::ValueArg<size_t> roiSizeXArg("x", "roi-size-x", "Size of ROI in x dimension", false, 53, "N>=1", cmd);
  TCLAP::ValueArg<size_t> roiSizeYArg("y", "roi-size-y", "Size of ROI in y dimension", false, 53, "N>=1", cmd);
  TCLAP::ValueArg<size_t> roiSizeZArg("z", "roi-size-z", "Size of ROI in z dimension", false, 41, "N>=1", cmd);
  TCLAP::ValueArg<unsigned int> maskValueArg("M", "mask-value",
                                             "The value of the mask that is inside the region of interest.", false, 1,
                                             "unsigned int", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string maskPath(maskArg.getValue()), outFilePath(outFileArg.getValue());
  const unsigned int numROIs(numROIsArg.getValue());
  const unsigned int maskValue(maskValueArg.getValue());

  typedef unsigned char MaskPixelType;
  typedef itk::Image<MaskPixelType, 3> MaskImageType;
  typedef MaskImageType::RegionType RegionType;
  itk::ImageFileReader<MaskImageType>::Pointer maskReader = itk::ImageFileReader<MaskImageType>::New();
  maskReader->SetFileName(maskPath);
  try {
    maskReader->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to Update mask reader." << std::endl
              << "Mask: " << maskPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  MaskImageType::SizeType roiSize;
  roiSize[0] = roiSizeXArg.getValue();
  roiSize[1] = roiSizeYArg.getValue();
  roiSize[2] = roiSizeZArg.getValue();
  try {
    const std::vector<RegionType> rois =
        ife::host::randomRegions<MaskImageType>(maskReader->GetOutput(), std::vector<int>(1, (int)maskValue), true,
                                                roiSize, numROIs, ife::host::SamplingSeed(), 0)[0];
    std::ofstream out(outFilePath.c_str());
    for (const RegionType &roi : rois) out << roi.GetIndex() << roi.GetSize() << '\n';
    out.flush();
    if (!out.good()) {
      std::cerr << "Error writing ROI info file" << std::endl;
      return EXIT_FAILURE;
    }
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to generate ROIs." << std::endl << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
