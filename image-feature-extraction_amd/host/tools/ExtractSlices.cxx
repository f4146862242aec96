// ExtractSlices -- slices of a volume along one axis, optionally restricted to the bounding box of
// a mask, one file per slice; the flags, printed lines, file names and index logic of the
// reference's tools/ExtractSlices.cxx (-i -o [-t nii.gz] [-m] [-s...] [-l...] [-w 0] [-d 0]
// [-a 2]).  Pixels are double.  The volume goes to the device once; each slice is one
// ife_extract_region of size 1 along the axis, which carries the reference's flip of the slice's
// second axis (z of the volume) when the axis is 0 or 1.  A slice is written as a volume
// (a, b, 1) of the two remaining axes in order; the suffix must be one the writer knows.
// Departure: the reference loops forever with -w above 1 and the default -d 0; that is refused.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <string>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Host/RegionFilters.h"

const std::string VERSION("0.1");

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Extract slices from an image.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Base path to output files", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> imageTypeArg("t", "type", "Image type suffix", false, "nii.gz", "suffix", cmd);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask. Must match image dimensions.", false, "", "path",
                                       cmd);
  TCLAP::MultiArg<unsigned int> sliceIndexArg("s", "slice-index", "Index of slices to extract", false, "unsigned int",
                                              cmd);
  TCLAP::MultiArg<double> sliceLocationArg("l", "slice-location", "Location of slices to extract", false, "[0,1]",
                                           cmd);
  TCLAP::ValueArg<unsigned int> sliceWindowArg(
      "w", "slice-window",
      "Size of window around slice locations/indices that should be extracted. This is used to extract slices "
      "neighboring those defined with slice-index and slice-location.",
      false, 0, "unsigned int", cmd);
  TCLAP::ValueArg<unsigned int> sliceStrideArg(
      "d", "slice-stride",
      "Stride to use when selecting slices in the slice-window. Must be positive if slice window > 1. Example usage: "
      "'--slice-window 10 --slice-stride 5' will extract the 5th preceding and following slices ",
      false, 0, "unsigned int", cmd);
  TCLAP::ValueArg<unsigned int> axisIndexArg("a", "axis-index", "Index of axis to extract", false, 2,
                                             "0:sagittal, 1:coronal, 2:axial", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue()), outBasePath(outArg.getValue()), suffix(imageTypeArg.getValue()),
      maskPath(maskArg.getValue());
  std::vector<unsigned int> indices(sliceIndexArg.getValue());
  const std::vector<double> locations(sliceLocationArg.getValue());
  const unsigned int sliceWindow(sliceWindowArg.getValue()), sliceStride(sliceStrideArg.getValue()),
      axisIndex(axisIndexArg.getValue());

  const unsigned int Dimension = 3;
  if (axisIndex >= Dimension) {
    std::cerr << "Axis index must be less than the number of dimensions" << std::endl;
    return EXIT_FAILURE;
  }
  if (sliceWindow / 2 > 0 && sliceStride == 0) {
    std::cerr << "Slice stride must be positive when the slice window is larger than 1" << std::endl;
    return EXIT_FAILURE;
  }
  if (suffix != "nii" && suffix != "nii.gz" && suffix != "mhd") {
    std::cerr << "Image type suffix must be nii, nii.gz or mhd" << std::endl;
    return EXIT_FAILURE;
  }

  typedef double PixelType;
  typedef itk::Image<PixelType, 3> ImageType;
  typedef ImageType::RegionType RegionType;
  itk::ImageFileReader<ImageType>::Pointer imageReader = itk::ImageFileReader<ImageType>::New();
  imageReader->SetFileName(imagePath);
  try {
    imageReader->Update();
    std::cout << "Origin " << imageReader->GetOutput()->GetOrigin() << std::endl
              << "Spacing " << imageReader->GetOutput()->GetSpacing() << std::endl
              << "Direction " << imageReader->GetOutput()->GetDirection() << std::endl;
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to read image." << std::endl
              << "Image path: " << imagePath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  RegionType region = imageReader->GetOutput()->GetLargestPossibleRegion();
  std::cout << "Region " << region << std::endl;

  if (!maskPath.empty()) {
    // the union of the boxes of all components is the box of the foreground: no labelling
    typedef itk::Image<float, 3> MaskType;   // != 0 as the reference's bool pixels
    itk::ImageFileReader<MaskType>::Pointer maskReader = itk::ImageFileReader<MaskType>::New();
    maskReader->SetFileName(maskPath);
    try {
      maskReader->Update();
      ife::host::same_size(*imageReader->GetOutput(), *maskReader->GetOutput(), "ExtractSlices");
      if (ife::host::mask_bounding_box(*maskReader->GetOutput(), region, "ExtractSlices") == 0) {
        std::cerr << "At least one connected components expected" << std::endl << "Got 0" << std::endl;
        return EXIT_FAILURE;
      }
      std::cout << "Region " << region << std::endl;
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed to read mask." << std::endl
                << "Mask path: " << maskPath << std::endl
                << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
  }

  if (!locations.empty()) {
    const double maxIndex = static_cast<double>(region.GetSize()[axisIndex]) - 1;
    for (size_t k = 0; k < locations.size(); ++k)
      if (locations[k] >= 0 && locations[k] <= 1)
        indices.push_back(static_cast<unsigned int>(std::round(locations[k] * maxIndex)));
  }
  if (indices.empty()) {
    indices.resize(region.GetSize()[axisIndex]);
    std::iota(indices.begin(), indices.end(), 0);
  } else {
    const unsigned int maxOffset = sliceWindow / 2;
    const unsigned int outOfBoundsIndex = (unsigned int)region.GetSize()[axisIndex];
    if (maxOffset > 0) {
      const std::vector<unsigned int> selectedIndices(indices);
      for (size_t k = 0; k < selectedIndices.size(); ++k) {
        const unsigned int idx = selectedIndices[k];
        for (unsigned int offset = sliceStride; offset <= maxOffset; offset += sliceStride) {
          const unsigned int before = idx - offset, after = idx + offset;   // unsigned: a wrap is caught below
          if (before < idx) indices.push_back(before);
          if (after > idx && after < outOfBoundsIndex) indices.push_back(after);
          if (offset + sliceStride < offset) break;   // the offset itself would wrap
        }
      }
    }
    std::sort(indices.begin(), indices.end());
    indices.erase(std::unique(indices.begin(), indices.end()), indices.end());
    if (indices.back() >= outOfBoundsIndex) {
      std::cerr << "Slice indices are outside bounds" << std::endl
                << "Largest requested index is " << indices.back() << std::endl
                << "Largest possible index is " << region.GetSize()[axisIndex] << std::endl;
      return EXIT_FAILURE;
    }
  }

  typedef itk::ExtractImageFilter<ImageType, ImageType> ExtractFilterType;
  ExtractFilterType::Pointer extractFilter = ExtractFilterType::New();
  extractFilter->SetDirectionCollapseToIdentity();
  extractFilter->SetInput(imageReader->GetOutput());
  extractFilter->SetDeviceResident(true);   // one upload for all slices
  // the reference flips the slice's second axis when the axis is 0 or 1: that is z of the volume
  itk::FixedArray<bool, 3> flipAxes;
  flipAxes[0] = false;
  flipAxes[1] = false;
  flipAxes[2] = axisIndex != 2;
  extractFilter->SetFlipAxes(flipAxes);
  itk::ImageFileWriter<ImageType>::Pointer writer = itk::ImageFileWriter<ImageType>::New();

  RegionType::SizeType size = region.GetSize();
  size[axisIndex] = 0;   // the collapsed axis
  for (size_t k = 0; k < indices.size(); ++k) {
    const unsigned int sliceIndex = indices[k];
    RegionType::IndexType index = region.GetIndex();
    index[axisIndex] += sliceIndex;
    extractFilter->SetExtractionRegion(RegionType(index, size));
    const std::string out = outBasePath + "axis-" + std::to_string(axisIndex) + "_absslice-" +
                            std::to_string(index[axisIndex]) + "_relslice-" + std::to_string(sliceIndex) + "." + suffix;
    writer->SetFileName(out);
    try {
      extractFilter->Update();
      writer->SetInput(extractFilter->GetOutput());
      writer->Update();
    } catch (itk::ExceptionObject &e) {
      std::cerr << "Failed to process." << std::endl
                << "Image: " << imagePath << std::endl
                << "Mask: " << maskPath << std::endl
                << "Out: " << out << std::endl
                << "ExceptionObject: " << e << std::endl;
      return EXIT_FAILURE;
    }
  }
  return EXIT_SUCCESS;
}
