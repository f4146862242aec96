// SampleROIs -- the voxels of every region of interest of a float image as one CSV row per
// region.  Flags, messages and output of the reference's tools/SampleROIs.cxx (-i -r -o [-R true];
// "Got N rois.", "ROI size [sx, sy, sz].", "ROI size differ: a | b" and failure where the boxes
// have different sizes; the values of a region in its raster order, x fastest, written with the
// stream's default formatting).  The reference runs RegionOfInterestImageFilter once per region
// (:151-167); here all regions are gathered in one call on the device (ife_extract_rois).
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/IO/ROIReader.h"
#include "ife/ROI/DeviceSampling.h"

const std::string VERSION("0.1");

int main(int argc, char *argv[]) {
  typedef float PixelType;
  TCLAP::CmdLine cmd("Sample ROIs from an image.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> roiArg("r", "roi-file",
                                      "Path to ROI file. If given the ROIs in this file will be used,"
                                      "otherwise ROIs will be generated.",
                                      false, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Path to output", true, "", "path", cmd);
  TCLAP::ValueArg<bool> roiHasHeaderArg("R", "roi-file-has-header", "Flag indicating if the ROI file has a header", false,
                                        true, "boolean", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), roiPath(roiArg.getValue()), outPath(outArg.getValue());
  const bool roiHasHeader(roiHasHeaderArg.getValue());

  typedef itk::Image<PixelType, 3> ImageType;
  typedef ImageType::SizeType SizeType;
  typedef ImageType::RegionType RegionType;
  itk::ImageFileReader<ImageType>::Pointer imageReader = itk::ImageFileReader<ImageType>::New();
  imageReader->SetFileName(imagePath);

  std::vector<RegionType> rois;
  SizeType roiSize;
  try {
    rois = ROIReader<RegionType>::read(roiPath, roiHasHeader);
    std::cout << "Got " << rois.size() << " rois." << std::endl;
    roiSize = rois.at(0).GetSize();
    for (const RegionType &roi : rois) {
      const SizeType &s = roi.GetSize();
      if (s[0] != roiSize[0] || s[1] != roiSize[1] || s[2] != roiSize[2]) {
        std::cout << "ROI size differ: " << roiSize << " | " << s << std::endl;
        return EXIT_FAILURE;
      }
    }
    std::cout << "ROI size " << roiSize << "." << std::endl;
  } catch (std::exception &e) {
    std::cerr << "Error reading ROIs" << std::endl
              << "roiPath: " << roiPath << std::endl
              << "exception: " << e.what() << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<PixelType> bag;  // one row per region, one column per voxel
  try {
    bag = ife::host::extractRegions<ImageType>(imageReader->GetOutput(), rois);
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to update roiFilter." << std::endl << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  const size_t cols = (size_t)(roiSize[0] * roiSize[1] * roiSize[2]);
  std::ofstream out(outPath.c_str());
  for (size_t i = 0; i < rois.size(); ++i) {
    for (size_t j = 0; j < cols; ++j) {
      out << bag[i * cols + j];
      if (j + 1 < cols) out << ",";
    }
    out << '\n';
  }
  out.flush();
  if (!out.good()) {
    std::cerr << "Error writing bag to file" << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
