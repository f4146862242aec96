// ImageBrowser -- the inspection tool run before GenerateROIs and MakeBag: which values occur in an
// image and how often ('s'), and how many random boxes of a size it takes to cover the region
// between two thresholds ('r'), the number one gives -n of those tools.  Flag, command loop and
// printed texts of the reference's tools/ImageBrowser.cxx (-i; 'q', 'i', 's', 'r' on stdin).  The
// image is read as float and uploaded once; both questions are answered on the device
// (ife/ROI/DeviceCoverage.h).  's' leaves NaN voxels out and says so on stderr, and prints -0 and
// +0 as one value.  'r' draws its 2000 boxes in one seeded call (IFE_SEED fixes the seed, unset it
// comes from std::random_device); a threshold range in which no voxel admits a box fails, where the
// reference would draw forever.  The end of stdin ends the loop like 'q'.
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/ROI/DeviceCoverage.h"
#include "ife/ROI/DeviceSampling.h"

const std::string VERSION("0.2");

static void EstimateROICoverageFromImage(ife::host::DeviceVolume &volume) {
  unsigned int x, y, z;
  float low, high;
  std::cout << "ROI size (x y z): ";
  std::cin >> x >> y >> z;
  std::cout << "Threshold for inclusion (low high): ";
  std::cin >> low >> high;
  if (!std::cin) throw itk::ExceptionObject("the ROI size and the thresholds could not be read", "ImageBrowser");

  // the sums of nSamplesPerRound of the reference: the rounds are cumulative
  const unsigned int nSamplesPerRound[] = {10, 10, 10, 10, 10, 50, 100, 100, 100, 100, 500, 1000};
  std::vector<int64_t> roundEnds;
  int64_t nROIs = 0;
  for (unsigned int nSamples : nSamplesPerRound) roundEnds.push_back(nROIs += nSamples);

  const int64_t size[3] = {(int64_t)x, (int64_t)y, (int64_t)z};
  const ife::host::Coverage c = volume.coverage(size, low, high, roundEnds, ife::host::SamplingSeed());
  for (size_t r = 0; r < roundEnds.size(); ++r)
    std::cout << "Visited " << c.visited[r] << " voxels. " << roundEnds[r] << " ROIs overlap " << c.hits[r] << "/"
              << c.regionSize << " = " << static_cast<double>(c.hits[r]) / static_cast<double>(c.regionSize)
              << std::endl;
}

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Information about an image.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue());

  typedef itk::Image<float, 3> ImageType;
  itk::ImageFileReader<ImageType>::Pointer reader = itk::ImageFileReader<ImageType>::New();
  reader->SetFileName(imagePath);

  const std::string commands =
      "'q' : quit\n'i' : Info about image shape\n's' : Summary statistics\n'r' : ROI overlap estimation\n";

  try {
    reader->Update();
    const ImageType *image = reader->GetOutput();
    ife::host::DeviceVolume volume(*image);

    char command = 'q';
    std::cout << commands << std::endl;
    do {
      if (!(std::cin >> command)) break;
      switch (command) {
        case 'i': {
          std::cout << "Size " << image->GetLargestPossibleRegion().GetSize() << std::endl;
          break;
        }
        case 's': {
          const ife::host::Census census = volume.census();
          float old = -1e12;
          for (const float val : census.values) {
            std::cout << '(' << old << ',' << val << "]\t|\t";
            old = val;
          }
          std::cout << '(' << old << ",inf)\t|\t" << std::endl;
          for (const uint32_t count : census.counts) std::cout << count << "\t|\t";
          std::cout << 0 << "\t|\t" << std::endl;  // the bin beyond the last value
          if (census.nan > 0) std::cerr << census.nan << " NaN voxels were left out." << std::endl;
          break;
        }
        case 'r': {
          EstimateROICoverageFromImage(volume);
          break;
        }
        case 'q':
          break;
        default:
          std::cout << "Unknown command" << std::endl << commands << std::endl;
      }
    } while (command != 'q');
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to process." << std::endl
              << "Image: " << imagePath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }

  std::cout << "Bye" << std::endl;
  return EXIT_SUCCESS;
}
