// ScaleSpaceFeatures -- the maximum over scales of gamma-normalised measures of the Hessian
// eigenvalues, and the scale at which each peaks (ife_scale_select; ours, the reference has no
// such tool).  Flags in the manner of ExtractFeatures: -i image -m mask -o prefix, -s sigma
// (repeatable), -k {laplacian,tube,plate,blob} (repeatable), -p {bright,dark}, -g gamma, -a alpha,
// -b beta, -c c.  For each measure it writes <prefix><Kind>Response.nii.gz (float) and
// <prefix><Kind>Scale.nii.gz (unsigned char: the index of the scale in the order given, 255 where
// no scale answered) with the geometry of the input image.  The mask is clamped to {0, 1} as
// ExtractFeatures clamps it.  IFE_DIFFERENTIAL=1 takes the eigenvalues from the differential
// normalized convolution; IFE_OUT_FILE_TYPE selects another file type, as for ExtractFeatures.
#include <cstdlib>
#include <iostream>

#include "tclap/CmdLine.h"

#include "ife/Host/ImageIO.h"
#include "ife/Host/LiteFilters.h"
#include "ife/Host/ScaleSelectImageFilter.h"

const std::string VERSION("0.1");

static std::string outFileType() {
  const char *e = std::getenv("IFE_OUT_FILE_TYPE");  // ".nii.gz", ".nii" or ".mhd"
  return e ? std::string(e) : std::string(".nii.gz");
}

int main(int argc, char *argv[]) {
  TCLAP::CmdLine cmd("Select, per voxel, the scale at which a measure of the Hessian eigenvalues peaks.", ' ', VERSION);
  TCLAP::ValueArg<std::string> imageArg("i", "image", "Path to image.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> maskArg("m", "mask", "Path to mask.", true, "", "path", cmd);
  TCLAP::ValueArg<std::string> outArg("o", "out", "Base output path", true, "", "path", cmd);
  TCLAP::MultiArg<float> scalesArg("s", "scale", "Scales for the Gauss applicability function", true, "double", cmd);
  TCLAP::MultiArg<std::string> kindsArg("k", "kind", "Measure: laplacian, tube, plate or blob", true, "name", cmd);
  TCLAP::ValueArg<std::string> polarityArg("p", "polarity", "bright (default) or dark structures", false, "bright",
                                           "bright|dark", cmd);
  TCLAP::ValueArg<float> gammaArg("g", "gamma", "Scale normalisation exponent (default 1)", false, 1.0f, "float", cmd);
  TCLAP::ValueArg<float> alphaArg("a", "alpha", "Plate / line sensitivity (default 0.5)", false, 0.5f, "float", cmd);
  TCLAP::ValueArg<float> betaArg("b", "beta", "Blob sensitivity (default 0.5)", false, 0.5f, "float", cmd);
  TCLAP::ValueArg<float> cArg("c", "structure", "Structure sensitivity c; required for tube, plate and blob", false,
                              0.0f, "float", cmd);
  try {
    cmd.parse(argc, argv);
  } catch (TCLAP::ArgException &e) {
    std::cerr << "Error : " << e.error() << " for arg " << e.argId() << std::endl;
    return EXIT_FAILURE;
  }
  const std::string imagePath(imageArg.getValue());
  const std::string maskPath(maskArg.getValue());
  const std::string outBasePath(outArg.getValue());
  const std::vector<float> scales(scalesArg.getValue());

  int polarity;
  if (polarityArg.getValue() == "bright") polarity = 1;
  else if (polarityArg.getValue() == "dark") polarity = -1;
  else {
    std::cerr << "Polarity must be bright or dark" << std::endl;
    return EXIT_FAILURE;
  }
  const char *kinds[4] = {"laplacian", "tube", "plate", "blob"};
  const char *kindNames[4] = {"Laplacian", "Tube", "Plate", "Blob"};
  std::vector<ife_scale_measure> measures;
  std::vector<std::string> names;
  bool given[4] = {false, false, false, false};
  for (const std::string &k : kindsArg.getValue()) {
    int kind = -1;
    for (int i = 0; i < 4; ++i)
      if (k == kinds[i]) kind = i;
    if (kind < 0) {
      std::cerr << "Unknown measure: " << k << " (laplacian, tube, plate, blob)" << std::endl;
      return EXIT_FAILURE;
    }
    if (given[kind]) {
      std::cerr << "Measure given twice: " << k << std::endl;
      return EXIT_FAILURE;
    }
    if (kind != IFE_SS_LAPLACIAN && !cArg.isSet()) {
      std::cerr << "-c is required for tube, plate and blob" << std::endl;
      return EXIT_FAILURE;
    }
    given[kind] = true;
    ife_scale_measure m;
    m.kind = kind;
    m.polarity = polarity;
    m.gamma = gammaArg.getValue();
    m.alpha = alphaArg.getValue();
    m.beta = betaArg.getValue();
    m.c = cArg.getValue();
    measures.push_back(m);
    names.push_back(kindNames[kind]);
  }

  typedef float PixelType;
  typedef unsigned char MaskPixelType;
  typedef itk::Image<PixelType, 3> ImageType;
  typedef itk::Image<MaskPixelType, 3> MaskType;

  typedef itk::ImageFileReader<ImageType> ReaderType;
  ReaderType::Pointer reader = ReaderType::New();
  reader->SetFileName(imagePath);
  typedef itk::ImageFileReader<MaskType> MaskReaderType;
  MaskReaderType::Pointer maskReader = MaskReaderType::New();
  maskReader->SetFileName(maskPath);

  typedef itk::ClampImageFilter<MaskType, MaskType> ClampFilterType;
  ClampFilterType::Pointer clampFilter = ClampFilterType::New();
  clampFilter->InPlaceOn();
  clampFilter->SetBounds(0, 1);

  typedef itk::ScaleSelectImageFilter<ImageType, MaskType> SelectFilterType;
  SelectFilterType::Pointer selectFilter = SelectFilterType::New();
  typedef itk::ImageFileWriter<SelectFilterType::ResponseImageType> ResponseWriterType;
  typedef itk::ImageFileWriter<SelectFilterType::ScaleImageType> ScaleWriterType;

  std::string outPath;
  try {
    clampFilter->SetInput(maskReader->GetOutput());
    selectFilter->SetInputImage(reader->GetOutput());
    selectFilter->SetInputMask(clampFilter->GetOutput());
    selectFilter->SetScales(scales);
    selectFilter->SetMeasures(measures);
    selectFilter->Update();
    for (unsigned int m = 0; m < measures.size(); ++m) {
      outPath = outBasePath + names[m] + "Response" + outFileType();
      ResponseWriterType::Pointer responseWriter = ResponseWriterType::New();
      responseWriter->SetFileName(outPath);
      responseWriter->SetInput(selectFilter->GetResponse(m));
      responseWriter->Update();
      outPath = outBasePath + names[m] + "Scale" + outFileType();
      ScaleWriterType::Pointer scaleWriter = ScaleWriterType::New();
      scaleWriter->SetFileName(outPath);
      scaleWriter->SetInput(selectFilter->GetScaleIndex(m));
      scaleWriter->Update();
    }
  } catch (itk::ExceptionObject &e) {
    std::cerr << "Failed to process." << std::endl
              << "Image: " << imagePath << std::endl
              << "Mask: " << maskPath << std::endl
              << "Out: " << outPath << std::endl
              << "ExceptionObject: " << e << std::endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
