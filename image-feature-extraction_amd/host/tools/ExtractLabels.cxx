// ExtractLabels -- the label of every region of interest: the mode of a label image inside the
// region.  Flags, messages and output of the reference's tools/ExtractLabels.cxx (-i -r [-R false]
// [-g ...] [-d -1] -o; "Got N rois."; one decimal label per line).  Ours, for the dense bag:
// -M/--roi-mask [-v/--roi-mask-value] [-x -y -z 41] as in MakeBagDense -- the regions are those of
// DenseROIGenerator on the ROI mask (!= 0 without -v, which matches a MakeBagDense run that
// generated from its clamped image mask; == value with -v, which matches MakeBagDense -M -v), the
// lines come in the row order of that bag, and no .ROIInfo is read or written.  Exactly one of -r
// and -M must be given.  Where two labels tie the smallest wins (include/ife_hip.h: the reference
// has no defined answer there).
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/IO/ROIReader.h"
#include "ife/Statistics/RegionLabels.h"

const std::string VERSION("0.1");

int main(int argc, char *argv[]) {
  typedef unsigned char PixelType;
  typedef unsigned short MaskPixelType;
  TCLAP::CmdLine cmd("Extract the mode from an image inside regions of interest.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> roiArg("r", "roi", "Path to roi. One of -r and -M is required.", false, "", "path",
                                      cmd);
  TCLAP::ValueArg<bool> roiHasHeaderArg("R", "roi-has-header", "Flag indicating if the ROI file has a header.", false,
                                        false, "boolean", cmd);
  TCLAP::MultiArg<unsigned int> ignoreArg("g", "ignore", "Values to ignore.", false, "unsigned char", cmd);
  TCLAP::ValueArg<int> dominantArg("d", "dominant",
                                   "If set, then this label will always be used if at least one pixel has the label.",
                                   false, -1, "unsigned char", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Output path", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> roiMaskArg("M", "roi-mask",
                                          "Path to ROI mask file. One region per voxel of the ROI mask whose box "
                                          "fits the image, in raster order (the regions of MakeBagDense).",
                                          false, "", "path", cmd);
  TCLAP::ValueArg<MaskPixelType> roiMaskValueArg("v", "roi-mask-value",
                                                 "Value in the ROI mask that should be used for inclusion. "
                                                 "If not given every non-zero value is used.",
                                                 false, 1, "MaskPixelType", cmd);
  TCLAP::ValueArg<size_t> roiSizeXArg("x", "roi-size-x", "Size of ROI in x dimension", false, 41, "N>=1", cmd);
  TCLAP::ValueArg<size_t> roiSizeYArg("y", "roi-size-y", "Size of ROI in y dimension", false, 41, "N>=1", cmd);
  TCLAP::ValueArg<size_t> roiSizeZArg("z", "roi-size-z", "Size of ROI in z dimension", false, 41, "N>=1", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), roiPath(roiArg.getValue()), outPath(outArg.getValue());
  const std::string roiMaskPath(roiMaskArg.getValue());
  const bool roiHasHeader(roiHasHeaderArg.getValue());
  const std::vector<unsigned int> ignoredLabels(ignoreArg.getValue());
  const int dominantLabel(dominantArg.getValue());
  if (roiArg.isSet() == roiMaskArg.isSet()) {
    std::cerr << "Error : exactly one of -r (--roi) and -M (--roi-mask) must be given" << std::endl;
    return EXIT_FAILURE;
  }

  if (dominantLabel > std::numeric_limits<PixelType>::max()) {
    std::cerr << "dominant label is to large" << std::endl
              << "dominantLabel" << dominantLabel << std::endl
              << "label max" << (int)std::numeric_limits<PixelType>::max() << std::endl;
    return EXIT_FAILURE;
  }
  std::vector<int> ignored;
  for (unsigned int ignoredLabel : ignoredLabels) {
    if (ignoredLabel > std::numeric_limits<PixelType>::max()) {
      std::cerr << "Ignored label is to large" << std::endl
                << "Ignored label" << ignoredLabel << std::endl
                << "label max" << (int)std::numeric_limits<PixelType>::max() << std::endl;
      return EXIT_FAILURE;
    }
    ignored.push_back((int)ignoredLabel);
  }

  typedef itk::Image<PixelType, 3> ImageType;
  typedef itk::Image<MaskPixelType, 3> MaskImageType;
  typedef ImageType::RegionType RegionType;
  itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
  reader->SetFileName(imagePath);
  try {
    reader->Update();
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to update reader" << std::endl
              << "imagePath: " << imagePath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<PixelType> labels;
  if (roiMaskArg.isSet()) {
    // the regions of the dense bag, without their boxes
    try {
      itk::ImageFileReader<MaskImageType>::Pointer roiMaskReader = itk::ImageFileReader<MaskImageType>::New();
      roiMaskReader->SetFileName(roiMaskPath);
      roiMaskReader->Update();
      const MaskImageType *rm = roiMaskReader->GetOutput();
      MaskImageType::Pointer genMask = MaskImageType::New();
      genMask->CopyInformation(rm);
      genMask->Allocate();
      const MaskPixelType value = roiMaskValueArg.getValue();
      for (uint64_t v = 0; v < rm->GetLargestPossibleRegion().GetNumberOfPixels(); ++v) {
        const MaskPixelType m = rm->GetBufferPointer()[v];
        genMask->GetBufferPointer()[v] = (roiMaskValueArg.isSet() ? m == value : m != 0) ? 1 : 0;
      }
      ImageType::SizeType roiSize;
      roiSize[0] = roiSizeXArg.getValue();
      roiSize[1] = roiSizeYArg.getValue();
      roiSize[2] = roiSizeZArg.getValue();
      labels = denseRegionLabels<ImageType, MaskImageType>(reader->GetOutput(), genMask.GetPointer(), roiSize, ignored,
                                                           dominantLabel);
      std::cout << "Got " << labels.size() << " rois." << std::endl;
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed to process" << std::endl
                << "ROI mask: " << roiMaskPath << std::endl
                << "Image->LargestPossibleRegion(): " << reader->GetOutput()->GetLargestPossibleRegion() << std::endl
                << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
  } else {
    std::vector<RegionType> rois;
    try {
      rois = ROIReader<RegionType>::read(roiPath, roiHasHeader);
      std::cout << "Got " << rois.size() << " rois." << std::endl;
    } catch (std::exception &e) {
      std::cerr << "Error reading ROIs" << std::endl
                << "roiPath: " << roiPath << std::endl
                << "exception: " << e.what() << std::endl;
      return EXIT_FAILURE;
    }
    try {
      labels = regionLabels<ImageType>(reader->GetOutput(), rois, ignored, dominantLabel);
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed to process" << std::endl
                << "Image->LargestPossibleRegion(): " << reader->GetOutput()->GetLargestPossibleRegion() << std::endl
                << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
  }

  std::ofstream out(outPath.c_str());
  for (size_t i = 0; i < labels.size(); ++i) out << (int)labels[i] << '\n';
  out.flush();
  if (!out.good()) {
    std::cerr << "Error writing to " << outPath << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
