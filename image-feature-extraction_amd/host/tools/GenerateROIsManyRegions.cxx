// GenerateROIsManyRegions -- GenerateROIs for several mask values in one run: -M may repeat, and
// every value gets a file <outfile><value>.ROIInfo of its own.  Flags, defaults and messages of the
// reference's tools/GenerateROIsManyRegions.cxx; without any -M it writes nothing and succeeds, as
// there.  All values go through one counting pass over the mask on the device, at most 32 per call
// (ife_random_rois with per_value); the draw stream of a value is its place in the list of -M.
// No file is written when one of a call's values admits no box ("Failed to generate ROIs.").
// IFE_SEED fixes the seed, unset it comes from std::random_device.
#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/ROI/DeviceSampling.h"

const std::string VERSION("0.2");

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Generate 3D ROIs.", ' ', VERSION);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outFileArg("o", "outfile", "Basepath for output files. <Maskvalue>.ROIInfo is appended",
                                          true, "", "path", cmd);
  TCLAP::ValueArg<unsigned int> numROIsArg("n", "num-rois", "Number of ROIs to sample", false, 50, "unsigned int", cmd);
  TCLAP::ValueArg<size_t> roiSizeXArg("x", "roi-size-x", "Size of ROI in x dimension", false, 53, "N>=1", cmd);
  TCLAP::ValueArg<size_t> roiSizeYArg("y", "roi-size-y", "Size of ROI in y dimension", false, 53, "N>=1", cmd);
  TCLAP::ValueArg<size_t> roiSizeZArg("z", "roi-size-z", "Size of ROI in z dimension", false, 41, "N>=1", cmd);
  TCLAP::MultiArg<unsigned int> maskValueArgs("M", "mask-value",
                                              "The value of the mask that is inside the region of interest.", false,
                                              "unsigned int", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string maskPath(maskArg.getValue()), outFilePath(outFileArg.getValue());
  const unsigned int numROIs(numROIsArg.getValue());
  const std::vector<unsigned int> maskValues(maskValueArgs.getValue());

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
  const uint64_t seed = ife::host::SamplingSeed();
  const size_t perCall = 32;  // the library's limit on the values of one counting pass
  for (size_t first = 0; first < maskValues.size(); first += perCall) {
    const size_t n = std::min(perCall, maskValues.size() - first);
    const std::vector<int> values(maskValues.begin() + first, maskValues.begin() + first + n);
    try {
      const std::vector<std::vector<RegionType> > rois = ife::host::randomRegions<MaskImageType>(
          maskReader->GetOutput(), values, true, roiSize, numROIs, seed, (uint32_t)first);
      for (size_t j = 0; j < n; ++j) {
        std::ostringstream name;
        name << outFilePath << maskValues[first + j] << ".ROIInfo";
        std::ofstream out(name.str().c_str());
        for (const RegionType &roi : rois[j]) out << roi.GetIndex() << roi.GetSize() << '\n';
        out.flush();
        if (!out.good()) {
          std::cerr << "Error writing ROI info file" << std::endl;
          return EXIT_FAILURE;
        }
      }
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed to generate ROIs." << std::endl << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
  }
  return EXIT_SUCCESS;
}
