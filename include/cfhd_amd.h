/* include/cfhd_amd.h -- C ABI of libcfhd_amd.so, the MI355X-native CineForm encode/decode core.
 *
 * The entry points are, symbol for symbol and argument for argument, the ones the reference SDK
 * exports for this path, so an application (or the reference's own Example/TestCFHD.cpp) that was
 * compiled against the reference headers links against this library unchanged.  Each declaration
 * cites the reference interface it replaces.  Handles are opaque; every function returns a
 * CFHD error code (0 = CFHD_ERROR_OKAY, Common/CFHDError.h:25-82).
 *
 * Scope: intra-frame encode of YUY2 / 2vuy (progressive and interlaced), YU64, v210 and the Avid 4:2:2 layouts avu8 / av16 / a106 / a214 / av28 (progressive)
 * -> YUV 4:2:2 10-bit; two-frame groups (CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP) from YUY2 / 2vuy (progressive and interlaced) and from YU64 / v210 / RG24 / BGRA / BGRa /
 * RG48 / b64a / RG64 / avu8 / av16 / a106 / a214 / av28 encoded as YUV 4:2:2 (progressive), through CFHD_EncodeSample and, a whole batch of groups per launch,
 * through the frame queue of cfhd_amd_batch_* (see cfhd_amd_batch_get_sequence_header below); RG48 / RG24 / BGRA / BGRa /
 * r210 / DPX0 / AB10 / AR10 / b64a -> RGB 4:4:4 12-bit, b64a -> RGBA 4:4:4:4 12-bit, BYR4 -> Bayer 12-bit; decode of 4:2:2 samples to
 * YUY2 / 2vuy (full and half resolution, interlaced samples too), RG48 / b64a / BGRA / BGRa (full and half resolution, interlaced samples too)
 * and YU64 (full resolution, progressive samples), RGB 4:4:4 samples to RG48 (and RG24 / BGRA / BGRa
 * at full resolution) and RGBA 4:4:4:4
 * samples to b64a at full and half resolution (DESIGN.md section 1 lists what each round added).  The Avid layouts are encoder inputs only: as decoder outputs
 * they hang off the reference's active-metadata colour engine, which is out of scope ("Refused").  Anything else
 * returns CFHD_ERROR_BADFORMAT (3) / CFHD_ERROR_BAD_RESOLUTION (11).
 * Both queues of the extension API have a device-memory side: the decode queue delivers its pictures into device memory the caller owns, packed or -- RG48 -- as
 * planar R, G, B tensors of u16 / f16 / f32 (cfhd_amd_decode_batch_set_device_pictures), the frame queue takes frames that lie in device memory
 * (cfhd_amd_batch_upload_device) or there as planar tensors (cfhd_amd_batch_upload_device_planar).  The plane layouts of both sides: RG48 as R, G, B, BYR4 mosaics as
 * the four planes of the 2 x 2 quad, the packed 4:2:2 formats YUY2 / 2vuy / YU64 as Y, Cb, Cr in the I422 convention (CFHD_AMD_PICTURES_YUV422_* /
 * CFHD_AMD_FRAMES_YUV422_*), and the formats that carry alpha, b64a / BGRA / BGRa, as R, G, B, A with the top row first (CFHD_AMD_PICTURES_RGBA_* /
 * CFHD_AMD_FRAMES_RGBA_*), each as integer, f16 or f32 elements.
 * There is no CPU fallback: without a HIP device the encode/decode calls return CFHD_ERROR_INTERNAL (6).
 */
#ifndef CFHD_AMD_H
#define CFHD_AMD_H
#include <stdint.h>
#include <stddef.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int CFHD_Error;                    /* Common/CFHDError.h:25 (enum, int sized) */
typedef uint32_t CFHD_PixelFormat;         /* Common/CFHDTypes.h:41  four character codes, e.g. 'YUY2' */
typedef int CFHD_EncodedFormat;            /* Common/CFHDTypes.h:231 0 = YUV 4:2:2, 1 = RGB 4:4:4, 2 = RGBA, 3 = Bayer */
typedef uint32_t CFHD_EncodingFlags;       /* Common/CFHDTypes.h:282 */
typedef int CFHD_EncodingQuality;          /* Common/CFHDTypes.h:200 1 = LOW .. 4 = FILMSCAN1 .. 6 = FILMSCAN3 */
typedef int CFHD_DecodedResolution;        /* Common/CFHDTypes.h:451 1 = full */
typedef uint32_t CFHD_DecodingFlags;       /* Common/CFHDTypes.h:489 */
typedef int CFHD_MetadataType;             /* Common/CFHDTypes.h:307 */
typedef int CFHD_MetadataTrack;            /* Common/CFHDTypes.h:405 */
typedef int CFHD_SampleInfoTag;            /* Common/CFHDTypes.h:182 */
typedef int CFHD_VideoSelect;              /* Common/CFHDTypes.h:417 */
typedef int CFHD_Stereo3DType;             /* Common/CFHDTypes.h:425 */
typedef int32_t CFHD_MetadataSize;
typedef struct cfhd_allocator CFHD_ALLOCATOR;   /* Common/CFHDAllocator.h (optional, may be NULL; unused here) */

typedef void *CFHD_EncoderRef;             /* Common/CFHDEncoder.h:54-57 */
typedef void *CFHD_MetadataRef;
typedef void *CFHD_EncoderPoolRef;
typedef void *CFHD_SampleBufferRef;
typedef void *CFHD_DecoderRef;             /* Common/CFHDDecoder.h:51 */

/* ---------------- synchronous encoder: EncoderSDK/CFHDEncoder.cpp ---------------- */
CFHD_Error CFHD_OpenEncoder(CFHD_EncoderRef *encoderRefOut, CFHD_ALLOCATOR *allocator);                 /* CFHDEncoder.h:255, .cpp:150 */
CFHD_Error CFHD_GetInputFormats(CFHD_EncoderRef encoderRef, CFHD_PixelFormat *inputFormatArray,
                                int inputFormatArrayLength, int *actualInputFormatCountOut);             /* CFHDEncoder.h:259 */
CFHD_Error CFHD_PrepareToEncode(CFHD_EncoderRef encoderRef, int frameWidth, int frameHeight,
                                CFHD_PixelFormat pixelFormat, CFHD_EncodedFormat encodedFormat,
                                CFHD_EncodingFlags encodingFlags, CFHD_EncodingQuality encodingQuality); /* CFHDEncoder.h:265, .cpp:261 */
CFHD_Error CFHD_SetEncodeLicense(CFHD_EncoderRef encoderRef, unsigned char *licenseKey);                 /* CFHDEncoder.h:274 (no-op) */
CFHD_Error CFHD_SetEncodeLicense2(CFHD_EncoderRef encoderRef, unsigned char *licenseKey, uint32_t *level);
CFHD_Error CFHD_EncodeSample(CFHD_EncoderRef encoderRef, void *frameBuffer, int framePitch);             /* CFHDEncoder.h:284, .cpp:319 */
CFHD_Error CFHD_GetSampleData(CFHD_EncoderRef encoderRef, void **sampleDataOut, size_t *sampleSizeOut);  /* CFHDEncoder.h:289, .cpp:382 */
CFHD_Error CFHD_CloseEncoder(CFHD_EncoderRef encoderRef);                                                /* CFHDEncoder.h:294 */

/* ---------------- encoder metadata: EncoderSDK/CFHDEncoderMetadata.cpp ---------------- */
CFHD_Error CFHD_MetadataOpen(CFHD_MetadataRef *metadataRefOut);                                          /* CFHDEncoder.h:313 */
CFHD_Error CFHD_MetadataAdd(CFHD_MetadataRef metadataRef, uint32_t tag, CFHD_MetadataType type,
                            size_t size, uint32_t *data, bool temporary);                                /* CFHDEncoder.h:316 */
CFHD_Error CFHD_MetadataAttach(CFHD_EncoderRef encoderRef, CFHD_MetadataRef metadataRef);                /* CFHDEncoder.h:324 */
CFHD_Error CFHD_MetadataClose(CFHD_MetadataRef metadataRef);                                             /* CFHDEncoder.h:327 */

/* ---------------- asynchronous encoder pool: EncoderSDK/CFHDEncoderPool.cpp ----------------
 * encoderThreadCount -> HIP streams (frames in flight on the GPU), jobQueueLength -> queued frames.
 * Samples come back in submission order (EncoderSDK/EncoderPool.cpp:297-380). */
CFHD_Error CFHD_CreateEncoderPool(CFHD_EncoderPoolRef *encoderPoolRefOut, int encoderThreadCount,
                                  int jobQueueLength, CFHD_ALLOCATOR *allocator);                        /* CFHDEncoder.h:338, Pool.cpp:103 */
CFHD_Error CFHD_GetAsyncInputFormats(CFHD_EncoderPoolRef encoderPoolRef, CFHD_PixelFormat *inputFormatArray,
                                     int inputFormatArrayLength, int *actualInputFormatCountOut);
CFHD_Error CFHD_PrepareEncoderPool(CFHD_EncoderPoolRef encoderPoolRef, uint_least16_t frameWidth, uint_least16_t frameHeight,
                                   CFHD_PixelFormat pixelFormat, CFHD_EncodedFormat encodedFormat,
                                   CFHD_EncodingFlags encodingFlags, CFHD_EncodingQuality encodingQuality); /* Pool.cpp:176 */
CFHD_Error CFHD_SetEncoderPoolLicense(CFHD_EncoderPoolRef encoderPoolRef, unsigned char *licenseKey);
CFHD_Error CFHD_SetEncoderPoolLicense2(CFHD_EncoderPoolRef encoderPoolRef, unsigned char *licenseKey, uint32_t *level);
CFHD_Error CFHD_AttachEncoderPoolMetadata(CFHD_EncoderPoolRef encoderPoolRef, CFHD_MetadataRef metadataRef);
CFHD_Error CFHD_StartEncoderPool(CFHD_EncoderPoolRef encoderPoolRef);                                    /* Pool.cpp:360 */
CFHD_Error CFHD_StopEncoderPool(CFHD_EncoderPoolRef encoderPoolRef);
CFHD_Error CFHD_EncodeAsyncSample(CFHD_EncoderPoolRef encoderPoolRef, uint32_t frameNumber, void *frameBuffer,
                                  intptr_t framePitch, CFHD_MetadataRef metadataRef);                    /* Pool.cpp:436 */
CFHD_Error CFHD_WaitForSample(CFHD_EncoderPoolRef encoderPoolRef, uint32_t *frameNumberOut,
                              CFHD_SampleBufferRef *sampleBufferRefOut);                                 /* Pool.cpp:475 */
CFHD_Error CFHD_TestForSample(CFHD_EncoderPoolRef encoderPoolRef, uint32_t *frameNumberOut,
                              CFHD_SampleBufferRef *sampleBufferRefOut);                                 /* Pool.cpp:520 */
CFHD_Error CFHD_GetEncodedSample(CFHD_SampleBufferRef sampleBufferRef, void **sampleDataOut, size_t *sampleSizeOut); /* Pool.cpp:557 */
CFHD_Error CFHD_ReleaseSampleBuffer(CFHD_EncoderPoolRef encoderPoolRef, CFHD_SampleBufferRef sampleBufferRef);       /* Pool.cpp:726 */
CFHD_Error CFHD_ReleaseEncoderPool(CFHD_EncoderPoolRef encoderPoolRef);

/* ---------------- decoder: DecoderSDK/CFHDDecoder.cpp ---------------- */
CFHD_Error CFHD_OpenDecoder(CFHD_DecoderRef *decoderRefOut, CFHD_ALLOCATOR *allocator);                  /* CFHDDecoder.h:203 */
CFHD_Error CFHD_GetOutputFormats(CFHD_DecoderRef decoderRef, void *samplePtr, size_t sampleSize,
                                 CFHD_PixelFormat *outputFormatArray, int outputFormatArrayLength, int *actualOutputFormatCountOut);
CFHD_Error CFHD_GetSampleInfo(CFHD_DecoderRef decoderRef, void *samplePtr, size_t sampleSize,
                              CFHD_SampleInfoTag tag, void *value, size_t buffer_size);                  /* CFHDDecoder.h:216 */
CFHD_Error CFHD_PrepareToDecode(CFHD_DecoderRef decoderRef, int outputWidth, int outputHeight, CFHD_PixelFormat outputFormat,
                                CFHD_DecodedResolution decodedResolution, CFHD_DecodingFlags decodingFlags,
                                void *samplePtr, size_t sampleSize, int *actualWidthOut, int *actualHeightOut,
                                CFHD_PixelFormat *actualFormatOut);                                      /* CFHDDecoder.h:224 */
CFHD_Error CFHD_GetPixelSize(CFHD_PixelFormat pixelFormat, uint32_t *pixelSizeOut);                      /* CFHDDecoder.h:244 */
CFHD_Error CFHD_GetImagePitch(uint32_t imageWidth, CFHD_PixelFormat pixelFormat, int32_t *imagePitchOut);/* CFHDDecoder.h:247 */
CFHD_Error CFHD_GetImageSize(uint32_t imageWidth, uint32_t imageHeight, CFHD_PixelFormat pixelFormat,
                             CFHD_VideoSelect videoselect, CFHD_Stereo3DType stereotype, uint32_t *imageSizeOut); /* CFHDDecoder.h:250 */
CFHD_Error CFHD_DecodeSample(CFHD_DecoderRef decoderRef, void *samplePtr, size_t sampleSize,
                             void *outputBuffer, int32_t outputPitch);                                   /* CFHDDecoder.h:262, .cpp:716 */
CFHD_Error CFHD_SetLicense(CFHD_DecoderRef decoderRef, const unsigned char *licenseKey);
CFHD_Error CFHD_SetActiveMetadata(CFHD_DecoderRef decoderRef, CFHD_MetadataRef metadataRef, unsigned int tag,
                                  CFHD_MetadataType type, void *data, unsigned int size);                /* CFHDDecoder.h:272 (accepted, ignored) */
CFHD_Error CFHD_ClearActiveMetadata(CFHD_DecoderRef decoderRef, CFHD_MetadataRef metadataRef);
CFHD_Error CFHD_GetThumbnail(CFHD_DecoderRef decoderRef, void *samplePtr, size_t sampleSize, void *outputBuffer,
                             size_t outputBufferSize, uint32_t flags, size_t *retWidth, size_t *retHeight, size_t *retSize); /* CFHDDecoder.cpp:1512 */
/* the same 1/8 x 1/8 10-bit RGB thumbnail through the encoder-side handles */
CFHD_Error CFHD_GetEncodeThumbnail(CFHD_EncoderRef encoderRef, void *samplePtr, size_t sampleSize, void *outputBuffer,
                                   size_t outputBufferSize, uint32_t flags, size_t *retWidth, size_t *retHeight, size_t *retSize); /* CFHDEncoder.cpp:593 */
CFHD_Error CFHD_GetSampleThumbnail(CFHD_SampleBufferRef sampleBufferRef, void *thumbnailBuffer, size_t bufferSize, uint32_t flags,
                                   uint_least16_t *actualWidthOut, uint_least16_t *actualHeightOut, CFHD_PixelFormat *pixelFormatOut,
                                   size_t *actualSizeOut);                                              /* CFHDEncoderPool.cpp:620 */
/* obsolete in the reference (use CFHD_GetSampleInfo); layout of Common/CFHDSampleHeader.h:32 */
typedef struct CFHD_SampleHeader { int encoded_format; int field_type; int width; int height; } CFHD_SampleHeader;
CFHD_Error CFHD_ParseSampleHeader(void *samplePtr, size_t sampleSize, CFHD_SampleHeader *sampleHeader);   /* CFHDDecoder.cpp:443 */
CFHD_Error CFHD_CloseDecoder(CFHD_DecoderRef decoderRef);                                                /* CFHDDecoder.h:300 */

/* ---------------- decoder-side metadata: DecoderSDK/CFHDMetadata.cpp ---------------- */
CFHD_Error CFHD_OpenMetadata(CFHD_MetadataRef *metadataRefOut);                                          /* CFHDMetadata.cpp:115 */
CFHD_Error CFHD_InitSampleMetadata(CFHD_MetadataRef metadataRef, CFHD_MetadataTrack track, void *sampleData, size_t sampleSize); /* :157 */
CFHD_Error CFHD_ReadMetadata(CFHD_MetadataRef metadataRef, unsigned int *tag, CFHD_MetadataType *type, void **data, CFHD_MetadataSize *size);
CFHD_Error CFHD_FindMetadata(CFHD_MetadataRef metadataRef, unsigned int tag, CFHD_MetadataType *type, void **data, CFHD_MetadataSize *size);
CFHD_Error CFHD_CloseMetadata(CFHD_MetadataRef metadataRef);                                             /* :1371 */

/* ---------------- extensions of this library (not in the reference ABI) ---------------- */
/* Batched, device-resident round trip used by bench.py: frames already in HBM -> samples -> frames in HBM. */
typedef struct cfhd_amd_batch cfhd_amd_batch;
/* nframes frames of one geometry travel through every stage together, one launch per stage (cfhd_batch.cpp).  The arguments are those of
 * CFHD_PrepareToEncode; mode 0: encode + decode back to the same pixel format, mode 1: encode only (the only mode for BYR4).
 * NULL for a quality word whose quantizer tables follow the size of the sample in front (cfhd_amd_quantizer_is_static answers 0): those streams go through
 * cfhd_amd_batch_create_stream below; this entry keeps refusing them, for callers that probe with it.
 * cfhd_amd_batch_create: 4:2:2 progressive round trip (YUY2 / 2vuy), kept for callers of the first release. */
cfhd_amd_batch *cfhd_amd_batch_create_ex(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags,
                                         int quality, int nframes, int nthreads, int mode);
cfhd_amd_batch *cfhd_amd_batch_create(int width, int height, uint32_t pixel_format, int quality, int nframes, int nthreads);
void cfhd_amd_batch_destroy(cfhd_amd_batch *batch);
int  cfhd_amd_batch_upload(cfhd_amd_batch *batch, int frame, const void *pixels, int pitch);   /* host frame -> HBM (outside any timed region) */
/* cfhd_amd_batch_upload for a frame that lies in HBM on the batch's device (a renderer's, PyTorch's, the decode queue's pictures: the caller vouches for the device):
 * the same frame index -- intra, group and stream batches -- and the same pitch rules, a negative pitch and the inputs walked as tightly packed rows whatever the
 * pitch (BYR4, BYR5, av28) included.  One strided device-to-device copy queued on the batch's stream, no staging, no host wait: the source is borrowed until the next
 * cfhd_amd_batch_wait / cfhd_amd_batch_roundtrip of the batch returns, and whatever produced it has completed before this call.  0; -1 for bad arguments (no batch, a
 * frame outside the batch, no pointer, a pitch whose magnitude is below the row bytes) or a pass in flight; another value for a device failure. */
int  cfhd_amd_batch_upload_device(cfhd_amd_batch *batch, int frame, const void *d_pixels, int pitch);
/* Frames first_frame .. first_frame + count - 1 of a batch whose pixel format is RG48 from planar tensors in HBM on the batch's device: what
 * cfhd_amd_decode_batch_set_device_pictures' PLANAR_* layouts are to the decode queue, for the frame queue (a renderer's or a model's output, the decode queue's own
 * planar pictures after some processing).  Every kind of batch that takes RG48 -- intra to 4:2:2 and to RGB 4:4:4, cfhd_amd_batch_create_groups, _create_stream,
 * _create_group_stream --, the frame indices with their per-frame meaning as for cfhd_amd_batch_upload_device.
 * Frame first_frame + i is read from d_frames + i * frame_stride: three planes, R, then G, then B, each `height` rows of `width` elements, rows row_pitch bytes apart,
 * planes height * row_pitch bytes apart -- the geometry of cfhd_amd_decode_batch_set_device_pictures.  A contiguous tensor (n, 3, H, W) is row_pitch = W * element
 * size, frame_stride = 3 * H * row_pitch.
 * One kernel launch (k_enc_collect) for the whole run, queued on the stream the pass runs on; no staging, no host wait.  The source is borrowed until the next
 * cfhd_amd_batch_wait / cfhd_amd_batch_roundtrip of the batch returns, whatever produced it has completed before this call, and it is never written.
 * Element -> RG48 word w.  CFHD_AMD_FRAMES_PLANAR_U16: w is the element.  _F32: t = x * 65535.0f, one IEEE single multiply; NaN gives 0; t is clamped to [0, 65535]
 * and rounded to nearest, ties to even -- so -0, everything negative and -inf give 0, everything >= 1 and +inf give 65535.  _F16: the binary16 value widened exactly
 * to single, subnormals kept, then the F32 rule.  These rules invert the delivery rules of cfhd_amd_decode_batch_set_device_pictures: a picture delivered as
 * PLANAR_U16 or PLANAR_F32 and collected in the same layout gives back every one of the 65 536 words w.  binary16 has 11 significant bits and cannot: what holds for
 * F16 is that a tensor collected as F16 and delivered as PLANAR_F16 again returns the binary16 bit pattern of every element that PLANAR_F16 delivery can produce.
 * 0; -1 with the reason in cfhd_amd_last_error(): no batch, a pass in flight, a batch whose input is not RG48, an unknown layout (0 included), count < 1 or a run
 * that leaves the batch, no pointer, a pointer, frame stride or row pitch that is no multiple of 16, a row pitch that is negative or below width * element size, a
 * frame stride below 3 * height * row_pitch; another value for a device failure.
 * cfhd_amd_batch_kernel_ms(batch, 20) is the HIP-event time of the k_enc_collect launches that fed the last completed pass (0 when none did),
 * cfhd_amd_batch_kernel_name(batch, 20) "k_enc_collect".
 * CFHD_AMD_FRAMES_BAYER_U16 / _F16 / _F32: the same for every batch whose input is BYR4 -- cfhd_amd_batch_create_ex mode 1, cfhd_amd_batch_create_bayer modes 0 and 1,
 * cfhd_amd_batch_create_stream -- and for no other (BYR5 is not served; a BYR4 batch takes no PLANAR_* layout, an RG48 batch no BAYER_* one).  A mosaic of W x H
 * photosites (the batch's width and height) is read as four planes of H / 2 rows of W / 2 elements: plane k = 2 * (row & 1) + (column & 1) holds the photosites at
 * that position of every 2 x 2 quad -- the codec does not know the CFA phase, the planes are named by position; for an RGGB mosaic they are R, G1, G2, B.  Rows
 * row_pitch bytes apart, planes (H / 2) * row_pitch apart: the geometry of CFHD_AMD_PICTURES_BAYER_*.  A contiguous tensor (n, 4, H / 2, W / 2) is row_pitch =
 * (W / 2) * element size, frame_stride = 4 * (H / 2) * row_pitch.  The element rules are the ones above, on the 16-bit photosite word, and so are the inversion
 * properties.  One launch of k_enc_collect_bayer per run (per chunk of a cut intra batch), timed under index 20; cfhd_amd_batch_kernel_name(batch, 20) answers
 * "k_enc_collect_bayer" for a BYR4 batch.  Refused as above, with W / 2 for the width and a frame stride below 4 * (H / 2) * row_pitch.
 * CFHD_AMD_FRAMES_YUV422_U8 / _U16 / _F16 / _F32: the same for every batch whose pixel format is YUY2, 2vuy or YU64 -- cfhd_amd_batch_create, _create_ex, _create_groups,
 * _create_stream, _create_group_stream; interlaced YUY2 / 2vuy included, the frame rows in their frame order -- and for no other (v210, the Avid layouts and the RGB
 * formats are refused with a text of their own; to a BYR4 batch the values are unknown layouts).  A frame of W x H pixels is read as three planes in the I422
 * convention, the geometry of CFHD_AMD_PICTURES_YUV422_*: Y, H rows of W elements row_pitch bytes apart, at 0; Cb, H rows of W / 2 elements row_pitch / 2 bytes apart,
 * at H * row_pitch; Cr, the same, at H * row_pitch + H * row_pitch / 2 -- always Y, Cb, Cr, whatever the packed order (Cb becomes byte 1 of YUY2's Y0 U Y1 V, byte 0
 * of 2vuy's U Y0 V Y1, word 3 of YU64's Y0 C1 Y1 C2; Cr byte 3, byte 2, word 1).  A contiguous frame is row_pitch = W * element size, frame_stride = 2 * H *
 * row_pitch.  _U8 exists for YUY2 and 2vuy only, _U16 for YU64 only: the element as it is.  _F16 / _F32: the rules above with the unit of the batch's own word,
 * 255 or 65535 (t = x * unit, NaN to 0, clamped to [0, unit], rounded to nearest even); no range scaling, no chroma offset.  The inversion properties: for the
 * 16-bit unit as above; for the 8-bit unit collect(deliver(b)) = b for all 256 bytes through U8, F32 and also F16 (the binary16 values of b / 255 are 256 distinct
 * numbers that come back within 0.063 of b).  One launch of k_enc_collect_yuv422 per run (per chunk of a cut intra batch), timed under index 20;
 * cfhd_amd_batch_kernel_name(batch, 20) answers "k_enc_collect_yuv422" for a batch of these three formats.  Refused as above, and: _U8 on a YU64 batch, _U16 on an
 * 8-bit one, a row pitch that is no multiple of 32 or below W * element size, a frame stride below 2 * H * row_pitch.
 * CFHD_AMD_FRAMES_RGBA_U8 / _U16 / _F16 / _F32: the same for every batch whose pixel format is b64a, BGRA or BGRa -- cfhd_amd_batch_create_ex to 4:2:2, RGB 4:4:4 and
 * RGBA 4:4:4:4, _create_groups, _create_stream, _create_group_stream -- and for no other (to every other batch the values are what they were before these layouts
 * existed: an unknown layout, or the text that batch has for every foreign value).  A frame of W x H pixels is read as four planes, R, then G, then B, then A, each H
 * rows of W elements, rows row_pitch bytes apart, planes H * row_pitch apart: the geometry of CFHD_AMD_PICTURES_RGBA_*.  A contiguous tensor (n, 4, H, W) is
 * row_pitch = W * element size, frame_stride = 4 * H * row_pitch.  The plane order is always R, G, B, A, whatever the packed order (b64a: the native 16-bit words A, R,
 * G, B; BGRA and BGRa: the bytes B, G, R, A), and the planes always have the top row first: BGRA, whose packed frame has the bottom row first, takes plane row r into
 * packed row H - 1 - r; BGRa and b64a keep their order.  _U8 exists for BGRA and BGRa only, _U16 for b64a only: the element as it is.  _F16 / _F32: the rules above
 * with the unit of the batch's own word, 255 or 65535.  Alpha is a component like the others: the packed byte or word, no companding, no premultiplication.  A batch
 * that encodes to 4:2:2 or RGB 4:4:4 still reads the A plane into the frame slot; the encoder drops it, as it does for an uploaded packed frame.  The inversion
 * properties are those of the YUV422 layouts: for the 8-bit unit collect(deliver(b)) = b for all 256 bytes through U8, F32 and F16; for the 16-bit unit U16 and F32
 * are exact for all 65 536 words and F16 is idempotent.  One launch of k_enc_collect_rgba per run (per chunk of a cut intra batch), timed under index 20;
 * cfhd_amd_batch_kernel_name(batch, 20) answers "k_enc_collect_rgba" for a batch of these three formats.  Refused as above, and: _U8 on a b64a batch, _U16 on an
 * 8-bit one, a row pitch below W * element size, a frame stride below 4 * H * row_pitch. */
enum { CFHD_AMD_FRAMES_PLANAR_U16 = 1, CFHD_AMD_FRAMES_PLANAR_F16 = 2, CFHD_AMD_FRAMES_PLANAR_F32 = 3 };      /* values equal to CFHD_AMD_PICTURES_PLANAR_* */
enum { CFHD_AMD_FRAMES_BAYER_U16 = 4, CFHD_AMD_FRAMES_BAYER_F16 = 5, CFHD_AMD_FRAMES_BAYER_F32 = 6 };         /* values equal to CFHD_AMD_PICTURES_BAYER_* */
enum { CFHD_AMD_FRAMES_YUV422_U8 = 7, CFHD_AMD_FRAMES_YUV422_U16 = 8, CFHD_AMD_FRAMES_YUV422_F16 = 9, CFHD_AMD_FRAMES_YUV422_F32 = 10 };      /* values equal to CFHD_AMD_PICTURES_YUV422_* */
enum { CFHD_AMD_FRAMES_RGBA_U8 = 11, CFHD_AMD_FRAMES_RGBA_U16 = 12, CFHD_AMD_FRAMES_RGBA_F16 = 13, CFHD_AMD_FRAMES_RGBA_F32 = 14 };          /* values equal to CFHD_AMD_PICTURES_RGBA_* */
int  cfhd_amd_batch_upload_device_planar(cfhd_amd_batch *batch, int first_frame, int count, const void *d_frames, size_t frame_stride, int row_pitch, int layout);
/* Frame `frame` as the batch holds it, in its packed input format, into out (rows `pitch` >= row bytes apart): the twin of cfhd_amd_batch_download_output for the
 * input side, for every kind of batch and input format (av28: the frame's one block as one row).  Waits for the stream the uploads run on.  0; -1 for bad arguments
 * or a pass in flight; another value for a device failure. */
int  cfhd_amd_batch_download_frame(cfhd_amd_batch *batch, int frame, void *out, int pitch);
long long cfhd_amd_batch_roundtrip(cfhd_amd_batch *batch);                                     /* one pass; total sample bytes, or < 0 */
/* The same pass as a slot of a frame queue (replaces the reference's EncoderPool job queue, EncoderSDK/EncoderPool.cpp:239-380): submit returns at once -- the whole
 * pass is queued on the batch's HIP streams, the decoder's stream waiting for the encoder's events; no host thread, no host wait inside the pass --, wait returns what
 * cfhd_amd_batch_roundtrip would have; batches in flight at the same time overlap on the GPU.  One pass per batch at a time: between submit and wait every other entry
 * point on that batch (roundtrip, upload, get_sample, get_sequence_header, download_output, kernel_ms, dx_stats) returns its error value without touching the batch; destroy waits first.
 * Encode-only batches in flight on one device take turns (their host copies hide behind the next batch's kernels), round-trip batches run free.  A process that keeps
 * several batches in flight should run with GPU_MAX_HW_QUEUES=16 in its environment (ROCm runtime, read at start-up: by default all HIP streams of a process share 4
 * hardware queues and the streams of several passes wait for each other). */
int  cfhd_amd_batch_submit(cfhd_amd_batch *batch);
/* The same pass fed from host memory: frame i at frames + i * frame_stride (rows `pitch` bytes apart) goes to HBM on the pass's own stream, the decoded pictures come back to
 * pictures + i * picture_stride (NULL: none) behind it; both buffers are borrowed until cfhd_amd_batch_wait returns.  Buffers registered with
 * cfhd_amd_register_host_buffer are copied by DMA as they are, plain ones are staged by the calling thread.  This is the pool semantics of the reference
 * (EncoderSDK/EncoderPool.cpp:239-295: frames in, samples out, nothing resident) for whole batches; bench.py's `host_fed` figure times it. */
int  cfhd_amd_batch_submit_host(cfhd_amd_batch *batch, const void *frames, size_t frame_stride, int pitch, void *pictures, size_t picture_stride, int picture_pitch);
long long cfhd_amd_batch_wait(cfhd_amd_batch *batch);
int  cfhd_amd_batch_get_sample(cfhd_amd_batch *batch, int frame, const void **data, size_t *size);
int  cfhd_amd_batch_download_output(cfhd_amd_batch *batch, int frame, void *out, int pitch);
/* Batches of two-frame groups: encoding_flags with CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP (optionally CFHD_ENCODING_FLAGS_YUV_INTERLACED), encoded_format 0, an even
 * nframes -- frames 2g and 2g + 1 form group g.  mode 1 takes every 4:2:2 input of the group encoder but RG24 / BGRA / BGRa (those: cfhd_amd_batch_create_groups
 * below); mode 0 those whose own format a group decodes to at full resolution (YUY2, 2vuy, YU64, v210, RG48, b64a; interlaced groups: YUY2, 2vuy).  NULL for anything else: an odd nframes, a quality whose group
 * tables follow the previous key sample (FILMSCAN2 / 3, LOW .. HIGH up to 1080p), CFHD_AMD_ENTROPY=host.  Every entry point keeps its meaning per frame index
 * (upload, submit_host, download_output: frame i); get_sample(2g) is group sample g, get_sample(2g + 1) the 24-byte P-frame sample behind it.  In pass k (counted from
 * 0) both carry frame number k * nframes + 2g + 1: the samples of consecutive passes are the stream one CFHD_EncodeSample handle writes when it is fed the same frames,
 * with the sequence header -- this call -- taken out.  A pass returns the sum of the sizes of its group samples; -9: a group sample reached the size at which the
 * reference codes bands as zeros (80 % of width x height x bytes per pixel + 64 KB), which the device stage does not do -- the other samples of the pass are complete.
 * cfhd_amd_batch_kernel_ms / _kernel_name of such a batch: 0 level 1 of all frames, 1 temporal step + middle wavelets, 2 top wavelet, 3 last level (+ conversion),
 * 4 middle wavelets + temporal step, 5 top wavelet, 12 k_dec_parse_group, 13 band decoder, 14 k_dec_lowpass (cfhd_batch.cpp).
 * Returns 0 and the 40-byte header, or -1 for a batch without groups (or one between submit and wait). */
int  cfhd_amd_batch_get_sequence_header(cfhd_amd_batch *batch, const void **data, size_t *size);
/* A batch of two-frame groups from any input: what cfhd_amd_batch_create_ex makes with encoded_format 0 and CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP (implied here, OR-ed into
 * encoding_flags) -- the same samples byte for byte --, and in addition groups from RG24 / BGRA / BGRa.  The reference marks those sources
 * CFEncode_Temporal_Quality_32: subband 7 of every channel (the lowpass band of the temporal highpass wavelet) is divided by 32 and coded in two passes of code set 18,
 * here on the device (k_ent_split_two_pass in front of the entropy coder's count stage; its time falls under cfhd_amd_batch_kernel_ms index 8, with k_ent_count).
 * mode 1: encode only; mode 0: round trip to the input's own format (k_dec_band_two_pass decodes that band; its time falls under index 13, the band decoder).
 * cfhd_amd_batch_create_ex keeps refusing the three inputs, for callers that probe with it.  NULL as there: an odd nframes, a quality whose group tables follow the
 * previous key sample, CFHD_AMD_ENTROPY=host, a width that is no multiple of 16, interlaced groups from anything but YUY2 / 2vuy, mode 0 for an input without a
 * decoder output (RG64, the Avid layouts), a geometry the device group decoder does not take.  Every other cfhd_amd_batch_* entry point is shared and keeps its meaning
 * per frame index; -9 keeps its meaning. */
cfhd_amd_batch *cfhd_amd_batch_create_groups(int width, int height, uint32_t pixel_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode);
/* One encoder's stream on the frame queue, rate feedback included.  The arguments are cfhd_amd_batch_create_ex's for intra frames, and every quality word
 * CFHD_PrepareToEncode takes for them is taken: also the words whose quantizer tables follow the size of the sample in front (cfhd_amd_quantizer_is_static answers 0:
 * MEDIUM and HIGH on 4:2:2 frames up to 1920 x 1080, FILMSCAN2 / FILMSCAN3 everywhere), which cfhd_amd_batch_create_ex keeps refusing, for callers that probe with it.
 * A batch made here is ONE encoder's stream: frame i of pass k (counted from 0) is call k * nframes + i + 1 of one CFHD_EncodeSample handle prepared with the same
 * arguments and fed the same frames, and its sample is that call's sample byte for byte -- quantizer tables, header, frame number, metadata.  The quantizer state is
 * carried from the last frame of a pass to the first of the next.  For a word whose tables stand still this is exactly cfhd_amd_batch_create_ex's batch, same samples,
 * same launches.  For the others a pass is coded on a guess of every frame's tables (the first pass: the first frame's; afterwards: the tables the pass before ended
 * with, frame by frame) and checked against the sizes that come back in cfhd_amd_batch_wait; the frames from the first wrong guess on are coded again, as often as it
 * takes -- n rounds at the most, one on material whose tables stand still, which is the rule (the bit-rate limiter moves beyond 110 - 150 Mbit/s at 30 fps, the
 * FILMSCAN2 / 3 limiter settles within about twenty frames).  cfhd_amd_batch_submit queues round 0 without a host wait, as for every batch; the further rounds run inside
 * cfhd_amd_batch_wait.  Every other cfhd_amd_batch_* entry point is shared and keeps its meaning per frame index (upload, roundtrip, submit, submit_host, wait,
 * get_sample, download_output, kernel_ms / kernel_name -- of the last round).  mode 0 / 1 as for cfhd_amd_batch_create_ex; in mode 0 the pictures are those of the
 * final samples (the decoder's half runs again when round 0 did not hold).
 * A pass that fails (-3: a sample that does not fit its buffer, ...) leaves the stream's quantizer state as it was when the pass began; its samples are not the
 * handle's, and the stream is not to be continued behind it -- make a new batch.  A stream's tail shorter than nframes is padded by the caller (repeat the last
 * frame): feedback only flows forward, so the samples of the real frames do not depend on the padding; drop the padding's samples.  Independent streams -- several
 * batches -- overlap in flight like any batches; the passes of one stream depend on each other and run one at a time.
 * NULL, with the reason in cfhd_amd_last_error(): whatever cfhd_amd_batch_create_ex refuses for reasons other than moving tables; nframes < 1;
 * CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP (groups: cfhd_amd_batch_create_groups, or cfhd_amd_batch_create_group_stream below for any tables); CFHD_AMD_ENTROPY=host; for words whose tables move, the
 * arrangements with host work inside a pass (CFHD_AMD_HANDOFF=host, CFHD_AMD_CHUNK). */
cfhd_amd_batch *cfhd_amd_batch_create_stream(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags,
                                             int quality, int nframes, int nthreads, int mode);
/* The group twin of cfhd_amd_batch_create_stream: one group encoder's stream on the frame queue, rate feedback included.  The arguments and the inputs served are
 * cfhd_amd_batch_create_groups' (the group flag implied, encoded format 4:2:2: every 4:2:2 input of the group encoder, RG24 / BGRA / BGRa with subband 7 coded in two
 * passes, interlaced groups from YUY2 / 2vuy; mode 1, and mode 0 where cfhd_amd_batch_create_groups serves it), and EVERY quality word CFHD_PrepareToEncode takes for
 * groups is taken -- also the words whose group tables follow the size of the key sample in front (cfhd_amd_quantizer_is_static with the group flag answers 0: LOW ..
 * HIGH up to 1920 x 1080, FILMSCAN2 / FILMSCAN3 everywhere), which cfhd_amd_batch_create_ex and cfhd_amd_batch_create_groups keep refusing.
 * A batch made here is ONE encoder's stream: with cfhd_amd_batch_get_sequence_header in front, the samples of consecutive passes -- get_sample(2g) group g,
 * get_sample(2g + 1) the 24-byte P-frame sample behind it -- are the stream of one CFHD_EncodeSample handle prepared with the same arguments and fed the same frames,
 * byte for byte: quantizer tables, headers, frame numbers, metadata.  The handle deals a group's tables on the call that opens it, from the size of the key sample in
 * front (the sequence header for the first group, the group sample in front afterwards), and quantizes both frames with them; the batch walks the same steps
 * (cfhd_gop.h gop_quant_group, the handle's own code).  The quantizer state is carried from the last group of a pass to the first of the next.  For a word whose group
 * tables stand still this is exactly cfhd_amd_batch_create_groups' batch, same samples, same launches.  For the others a pass is coded on a guess of every group's
 * tables (the first pass: the first group's; afterwards: the tables the pass before ended with, group by group) and checked against the sizes that come back in
 * cfhd_amd_batch_wait; the groups from the first wrong guess on are coded again as a window of the batch, as often as it takes -- nframes / 2 rounds at the most, one
 * where the tables stand still.  Every other cfhd_amd_batch_* entry point is shared and keeps its meaning per frame index (upload, roundtrip, submit, submit_host,
 * wait, get_sample, download_output, kernel_ms / kernel_name -- of the last round); in mode 0 the pictures are those of the final samples.
 * A pass that fails (-3: a sample that does not fit its buffer, -8: a peak table the device stage cannot write, -9: a group at the size where the reference codes
 * bands as zeros) commits nothing: the carried state is the one the pass began with; its samples are not the handle's, and the stream is not to be continued
 * behind it.  A tail shorter than nframes is padded by the caller, as for cfhd_amd_batch_create_stream.
 * NULL, with the reason in cfhd_amd_last_error(): whatever cfhd_amd_batch_create_groups refuses for reasons other than moving tables; an odd nframes, or nframes < 2;
 * CFHD_AMD_ENTROPY=host; for words whose tables move, CFHD_AMD_HANDOFF=host. */
cfhd_amd_batch *cfhd_amd_batch_create_group_stream(int width, int height, uint32_t pixel_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode);
/* Bayer mosaics on the frame queue, both ways.  pixel_format BYR4 or BYR5 (the encoded format is Bayer, implied), the other arguments as for
 * cfhd_amd_batch_create_ex.  mode 1 is exactly cfhd_amd_batch_create_ex's batch: the same samples, the same launches.  mode 0 -- BYR4 only -- adds the decode back to
 * the BYR4 mosaic: picture i is what CFHD_DecodeSample gives for get_sample(i) with output BYR4 at full resolution, byte for byte (16-bit photosites, no dither).
 * Passes of 4 frames of 1080p-equivalent work and more (a 3840 x 2160 mosaic is one) write the mosaic straight from the last wavelet level (k_inv_bayer_strip);
 * smaller ones and CFHD_AMD_INVERSE=tile run the handle's pair k_inv_packed16 + k_bayer_to_byr4 -- the same bytes.  Every other cfhd_amd_batch_* entry point is shared and keeps its meaning per frame index (upload,
 * upload_device, roundtrip, submit, submit_host, wait, get_sample, download_output: the mosaic, width x height photosites in rows of 2 * width bytes; kernel_ms /
 * kernel_name 3..5 and 12..14 as for every round-trip batch, 3 naming the last-level kernel that ran).
 * NULL, with the reason in cfhd_amd_last_error(): an input that is no Bayer mosaic; BYR5 at mode 0 (no decoder output exists); a quality word whose tables follow
 * the sample sizes (as cfhd_amd_batch_create_ex: a Bayer stream with rate feedback is not built); whatever CFHD_PrepareToEncode or cfhd_amd_batch_create_ex refuses
 * otherwise.  cfhd_amd_batch_create_ex and cfhd_amd_batch_create_stream keep refusing mode 0 for Bayer inputs, for callers that probe with them. */
cfhd_amd_batch *cfhd_amd_batch_create_bayer(int width, int height, uint32_t pixel_format, uint32_t encoding_flags, int quality, int nframes, int nthreads, int mode);
/* The last completed pass of a stream batch: out[0] encode rounds (>= 1), out[1] frames coded over all rounds (>= nframes; a group stream: even), out[2] frames whose
 * tables differ from those of the frame in front (frame 0: from the last frame of the pass before; in pass 0 it counts 0) -- a group stream: groups, likewise.  0, or
 * -1 for a batch not made by cfhd_amd_batch_create_stream / cfhd_amd_batch_create_group_stream, before its first pass has completed, and between submit and wait. */
int  cfhd_amd_batch_stream_stats(cfhd_amd_batch *batch, int out[3]);
float cfhd_amd_batch_kernel_ms(cfhd_amd_batch *batch, int which);                              /* HIP-event time of the kernels of the last pass */
const char *cfhd_amd_batch_kernel_name(cfhd_amd_batch *batch, int which);                      /* which 0..5: the transform kernel behind that time; 20: "k_enc_collect" */
double cfhd_amd_batch_stage_seconds(cfhd_amd_batch *batch, int which);
/* The level-1 transform kernel of a prepared encoder handle's next CFHD_EncodeSample, intra frame or two-frame group ("" when the handle is not prepared). */
const char *cfhd_amd_encoder_kernel_name(CFHD_EncoderRef encoderRef);
int  cfhd_amd_batch_dx_stats(cfhd_amd_batch *batch, uint32_t *out16);
/* Whether the quantizer tables of these CFHD_PrepareToEncode arguments stay put from frame to frame (1), or follow the size of the previous sample (0: rate feedback --
 * FILMSCAN2 / FILMSCAN3, LOW .. HIGH up to 1080p -- which cfhd_amd_batch_create_ex refuses and CFHD_EncodeSample applies per frame); -1: arguments no encoder takes. */
int  cfhd_amd_quantizer_is_static(int width, int height, uint32_t pixel_format, int encoded_format, uint32_t encoding_flags, int quality);
/* ---------------- the decode queue: batches of samples from any encoder, parsed and decoded on the GPU (cfhd_decode_queue.hip) ----------------
 * What cfhd_amd_batch_* is to a caller who has just encoded, for a caller who holds a clip: nsamples samples a pass, one launch per stage for all of them, no host
 * tag walk and no device wait per picture.  Progressive and interlaced 4:2:2, RGB 4:4:4 and RGBA 4:4:4:4 samples, to every output and resolution CFHD_DecodeSample
 * serves for them; streams of two-frame groups through cfhd_amd_decode_batch_create_groups, Bayer samples (to BYR4) through cfhd_amd_decode_batch_create_bayer below. */
typedef struct cfhd_amd_decode_batch cfhd_amd_decode_batch;
/* Prepares from one complete intra sample, as CFHD_PrepareToDecode prepares a handle: geometry, encoded format, precision, scan and colour space are the first
 * sample's, output_format / decoded_resolution those of CFHD_PrepareToDecode.  NULL, with the reason in cfhd_amd_last_error(), for whatever CFHD_PrepareToDecode or
 * CFHD_DecodeSample refuses for that sample, output and resolution (the sample is decoded once on a handle of its own to find out), for group samples, P-frame samples,
 * sequence headers, Bayer samples, samples with an UNCOMPRESS chunk, under CFHD_AMD_ENTROPY=host, for nsamples < 1 or nsamples x channels > 65 535.  The batch lives on
 * the device a cfhd_amd_batch_create_ex of the same thread would. */
cfhd_amd_decode_batch *cfhd_amd_decode_batch_create(const void *first_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int nsamples);
/* The same batch for a stream of two-frame groups (CFHD_ENCODING_FLAGS_YUV_2FRAME_GOP, progressive or interlaced, from the reference's encoder, a camera or
 * CFHD_EncodeSample).  Prepares from one complete group sample (TAG_SAMPLE, type 2), the way a CFHD_DecodeSample handle is prepared on the first group of a stream;
 * every other entry point is shared and keeps its meaning per sample / picture index.  A pass carries count samples, count even and <= 2 * ngroups (an odd count: -1):
 * entry 2g is group sample g, entry 2g + 1 the P-frame sample behind it; picture 2g is the group's first frame, picture 2g + 1 its second.  Sequence headers are not
 * passed: a reader skips them.  What submit_host / submit_device say about alignment, registered spans, borrowed buffers, "exactly count pictures are written" and the
 * dither seed of pass k holds unchanged.
 * Every pair is judged alone: status[2g] and status[2g + 1] are what CFHD_DecodeSample returns for those two samples, in that order, on a handle prepared on the first
 * group sample that has no group behind it yet.  The picture of a sample that failed is zero, and so is that of a sample the handle answers CFHD_ERROR_OKAY for without
 * writing one (a sequence header passed as a sample).  Final on the device: a group the device parser refuses as a bad sample, with the P-frame sample behind it (no
 * picture without its group).  Decoded as a pair by the handle inside wait: a pair with a sample the device stage does not place (a group longer than
 * width x display height x 8 + 128 KB, a P-frame sample longer than 1 KB, a size that is no multiple of 4), a group whose scan or colour-space tag differs from the
 * first sample's, a follower that is not a plain P-frame sample, a group only the host decides and -- when any code stream of the pass is damaged -- every pair the
 * parser passed.
 * NULL, with the reason in cfhd_amd_last_error(): whatever CFHD_PrepareToDecode or CFHD_DecodeSample refuses for that sample, output and resolution, with the same text
 * (an interlaced group to YU64 at full resolution, the widths an output needs, quarter resolution); a sequence header, a P-frame sample or an intra sample as first
 * sample; CFHD_AMD_ENTROPY=host; ngroups < 1 or 6 x ngroups > 65 535; a geometry the device's group decoder does not take (such streams stay with CFHD_DecodeSample).
 * cfhd_amd_decode_batch_kernel_ms / _kernel_name of such a batch: 0 k_dec_ingest, 1 k_dec_parse_group, 2 the band decoder (every kernel of it, k_dec_band_two_pass --
 * subband 7 of the groups from 8-bit RGB sources -- included), 3 k_dec_lowpass, 4 / 5 / 6 the three inverse stages in launch order (the last with the output
 * conversion), 7 k_dec_blank; kernel_ms alone also answers 8: k_dec_band_two_pass by itself. */
cfhd_amd_decode_batch *cfhd_amd_decode_batch_create_groups(const void *first_group_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int ngroups);
/* The same batch for Bayer intra samples (CineForm RAW, from any encoder), decoded to what CFHD_DecodeSample serves for them: the BYR4 mosaic at full resolution,
 * no demosaic.  Prepares from one complete Bayer intra sample with the gates of cfhd_amd_decode_batch_create (CFHD_PrepareToDecode, then the first sample once through
 * CFHD_DecodeSample on the batch's own handle); cfhd_amd_decode_batch_create itself keeps refusing Bayer samples, for callers that probe with it.  Every other entry
 * point is shared and keeps its meaning: cfhd_amd_decode_batch_geometry answers the mosaic -- twice the sample's (component plane) width and rows, row_bytes =
 * 2 * width --; submit_host, submit_device, wait and download_output work as for any batch; status[i] is what CFHD_DecodeSample returns for sample i, the picture of
 * a sample that failed is zero, and the slow path inside wait is the handle's; every picture equals the handle's byte for byte (16-bit photosites, no dither).
 * cfhd_amd_decode_batch_set_device_pictures takes CFHD_AMD_PICTURES_PACKED -- the mosaic as it is -- and CFHD_AMD_PICTURES_BAYER_U16 / _F16 / _F32 -- the mosaic as four
 * planes, one per position of the 2 x 2 quad; the PLANAR_* layouts stay refused (the output is not RG48).
 * cfhd_amd_decode_batch_kernel_ms / _kernel_name: indices 0 .. 9 keep their meaning; 6 names the last level that ran -- "k_inv_bayer_strip", the mosaic written
 * straight from the last wavelet level (passes of 4 frames of 1080p-equivalent work and more -- a 3840 x 2160 mosaic is one --, or CFHD_AMD_INVERSE=strip), or
 * "k_inv_packed16+k_bayer_to_byr4", the handle's pair (smaller passes, or CFHD_AMD_INVERSE=tile); both give the same bytes.
 * NULL, with the reason in cfhd_amd_last_error(): a first sample that is not a Bayer intra sample; an output other than BYR4; half or quarter resolution;
 * CFHD_AMD_ENTROPY=host; nsamples < 1 or 4 x nsamples > 65 535; whatever CFHD_PrepareToDecode or CFHD_DecodeSample refuses for that sample. */
cfhd_amd_decode_batch *cfhd_amd_decode_batch_create_bayer(const void *first_sample, size_t first_size, uint32_t output_format, int decoded_resolution, int nsamples);
/* Thumbnails of a batch of samples: the 1/8 x 1/8 picture CFHD_GetThumbnail makes of each, straight from the raw level-3 lowpass words of the sample -- no entropy
 * decoder and no inverse transform run.  Prepares from one complete intra sample of encoded format 4:2:2, RGB 4:4:4 or RGBA 4:4:4:4, progressive or interlaced (a
 * batch serves both scans).  The output is fixed to what CFHD_GetThumbnail writes: W8 x H8 pixels, one big-endian longword a pixel, r << 22 | g << 12 | b << 2 ("DPX0"),
 * W8 = (width + 7) / 8 and H8 = (height + 7) / 8 of the first sample's header.  Every other entry point is shared and keeps its meaning:
 * cfhd_amd_decode_batch_geometry answers W8, H8 and row_bytes = 4 x W8; submit_host, submit_device, wait, download_output, set_device_pictures and destroy work as for
 * any batch, one pass per batch at a time, several batches in flight.  A pass is k_dec_ingest, k_dec_parse and k_dec_thumbnail on the batch's one stream, then the
 * delivery; no host wait inside.  Every picture equals CFHD_GetThumbnail's byte for byte.
 * Device memory: the sample slots (width x height x bytes per pixel of the sample's 16-bit picture + 64 KB each: about 4 MB for 1080p 4:2:2), the parser's tables,
 * the verdicts and the small pictures (4 x W8 x H8 bytes each); as much as the slots again once submit_host has been used (the samples' way in).  No coefficient
 * pyramid, no full-size picture and no chunk index: a decode batch of the same samples holds about 30 MB a sample.
 * status[i] of wait is what CFHD_GetThumbnail returns for sample i on any decoder handle, with one addition: a sample whose thumbnail would not have the batch's
 * W8 x H8 gets CFHD_ERROR_BADSAMPLE.  The picture of a sample whose status is not CFHD_ERROR_OKAY is zeros -- in the batch's buffer, in host delivery and in the caller's
 * device memory.  Samples the device stage places and whose tag stream the device parser passes are final on the GPU, whatever their scan flag and colour-space tag
 * (a thumbnail depends on neither); the others -- longer than a slot, a size that is no multiple of 4, anything the parser does not pass, such as an RGB 4:4:4 sample
 * of the same geometry in a 4:2:2 batch -- get status and picture from CFHD_GetThumbnail on their bytes inside wait.
 * cfhd_amd_decode_batch_set_device_pictures takes CFHD_AMD_PICTURES_PACKED -- the DPX0 words as they are -- and CFHD_AMD_PICTURES_RGB10_U16 / _F16 / _F32 (below); every
 * other layout is refused.  cfhd_amd_decode_batch_kernel_ms / _kernel_name: 0 k_dec_ingest, 1 k_dec_parse, 6 k_dec_thumbnail (the place of the last level), 9 the
 * deliver kernel while a layout is set; 0 / "" for every other index.
 * NULL, with the reason in cfhd_amd_last_error(): no first sample; nsamples < 1 or > 65 535 (the pictures are a grid dimension); group samples, P-frame samples and
 * sequence headers; Bayer samples (the reference makes their thumbnail by a quarter-resolution decode; CFHD_GetThumbnail answers CFHD_ERROR_BADFORMAT); a sample with
 * an UNCOMPRESS chunk; a first sample CFHD_GetThumbnail refuses; an odd W8 (CFHD_GetThumbnail writes even widths only); CFHD_AMD_ENTROPY=host. */
cfhd_amd_decode_batch *cfhd_amd_decode_batch_create_thumbnails(const void *first_sample, size_t first_size, int nsamples);
/* Waits for a pass in flight, then frees the batch. */
void cfhd_amd_decode_batch_destroy(cfhd_amd_decode_batch *batch);
/* One decoded picture: width x height pixels in rows of row_bytes bytes (any of the three may be NULL).  0, or -1. */
int  cfhd_amd_decode_batch_geometry(cfhd_amd_decode_batch *batch, int *width, int *height, int *row_bytes);
/* Starts a pass and returns at once: sample i is sizes[i] bytes at base + offsets[i] -- any byte alignment, any order, gaps allowed --, count <= nsamples; picture i goes
 * to pictures + i * picture_stride in rows picture_pitch apart (NULL: the pictures stay in HBM for cfhd_amd_decode_batch_download_output).  Exactly count pictures are
 * written, row_bytes of every row and nothing behind them.  Both buffers are borrowed until cfhd_amd_decode_batch_wait returns (offsets / sizes are copied).  A span
 * inside a buffer registered with cfhd_amd_register_host_buffer travels as one DMA as it lies; anything else is packed into the batch's pinned memory inside this call,
 * before the first launch -- the only host work of a pass: by the calling thread and, for passes of more than 8 samples, up to seven short-lived helper threads it joins
 * before it launches anything (wait copies pictures out of pinned memory into a plain picture buffer the same way).  Several decode batches in flight overlap on the GPU; one pass per batch at a time: between submit and
 * wait every other entry point on that batch returns its error value (-1, 0, ""), destroy waits first.  0, -1 for bad arguments, < -1 for a device failure.
 * 8-bit outputs: the dither seed of pass k (counted from 0 per batch) is 0xA511E9B3 * (k + 1), the rule of cfhd_amd_batch_submit's round trip -- CFHD_DecodeSample's
 * n-th call uses 0x2545F491 * n, so such pictures agree with the handle's to within the one dither step, all others byte for byte. */
int  cfhd_amd_decode_batch_submit_host(cfhd_amd_decode_batch *batch, const void *base, const size_t *offsets, const size_t *sizes, int count,
                                       void *pictures, size_t picture_stride, int picture_pitch);
/* The same for samples that already lie in HBM on the batch's device: sample i at d_base + offsets[i] (offsets, sizes: host arrays; every sample inside
 * [d_base, d_base + span_bytes), else -1).  The library reads the 16-byte aligned blocks that hold bytes of [d_base, d_base + span_bytes) -- its 16-byte hull -- and
 * nothing else, until wait returns.  The pictures stay in HBM. */
int  cfhd_amd_decode_batch_submit_device(cfhd_amd_decode_batch *batch, const void *d_base, size_t span_bytes, const size_t *offsets, const size_t *sizes, int count);
/* Names the device memory every later pass of the batch -- submit_host and submit_device, intra batches and group batches -- delivers its pictures into: picture i of a
 * pass at d_pictures + i * picture_stride, written by k_dec_deliver behind the pass's last kernel on the batch's stream.  d_pictures = NULL switches delivery off
 * again (the other arguments are ignored).  The memory lies on the batch's device -- the caller vouches for that, as for d_base of submit_device --, is borrowed from
 * submit until cfhd_amd_decode_batch_wait returns, and the caller's own work on it has completed before it submits; when wait has returned the pictures are complete
 * and visible to any stream.  Host delivery (`pictures` of submit_host) and cfhd_amd_decode_batch_download_output work unchanged beside it, the dither seed of pass k
 * is unchanged, and what the memory holds agrees with status[i] of wait as download_output does: zeros (0.0) for a sample that failed, the handle's picture for one the
 * handle decoded inside wait.
 * CFHD_AMD_PICTURES_PACKED: the batch's own output format and resolution, whatever it was created with -- `height` rows of `row_bytes` bytes
 * (cfhd_amd_decode_batch_geometry), picture_pitch bytes apart.
 * CFHD_AMD_PICTURES_PLANAR_U16 / _F16 / _F32: a batch created with output RG48 only (full or half resolution; 4:2:2, RGB 4:4:4 and RGBA 4:4:4:4 samples, progressive and
 * interlaced groups).  A picture is three planes, R, then G, then B, each `height` rows of `width` elements, rows picture_pitch bytes apart, planes height * picture_pitch
 * bytes apart: a contiguous tensor (n, 3, H, W) is picture_pitch = W * element size, picture_stride = 3 * H * W * element size.  For the RG48 word w: U16 is w; F32 is
 * (float)w * (1.0f / 65535.0f), one IEEE single multiply; F16 is that value rounded to nearest-even to binary16, subnormals kept.
 * CFHD_AMD_PICTURES_BAYER_U16 / _F16 / _F32: a batch made by cfhd_amd_decode_batch_create_bayer only (to every other batch these values are unknown layouts).  The
 * mosaic of W x H photosites (cfhd_amd_decode_batch_geometry) is four planes of H / 2 rows of W / 2 elements: plane k = 2 * (row & 1) + (column & 1) holds the
 * photosites at that position of every 2 x 2 quad -- the codec does not know the CFA phase, the planes are named by position; for an RGGB mosaic they are R, G1, G2,
 * B.  Rows picture_pitch bytes apart, planes (H / 2) * picture_pitch apart: a contiguous tensor (n, 4, H / 2, W / 2) is picture_pitch = (W / 2) * element size,
 * picture_stride = 4 * (H / 2) * picture_pitch.  The element rules are the RG48 ones on the 16-bit photosite word.  Written by k_dec_deliver_bayer in place of
 * k_dec_deliver (cfhd_amd_decode_batch_kernel_name(batch, 9) answers it while such a layout is set; kernel_ms index 9 times it).
 * CFHD_AMD_PICTURES_YUV422_U8 / _U16 / _F16 / _F32: every batch whose output is YUY2, 2vuy or YU64 -- intra batches of progressive and interlaced samples, group
 * batches, full and half resolution -- and no other (v210 and the RGB outputs are refused with a text of their own; to a Bayer batch the values are unknown layouts).
 * The picture of W x H pixels (cfhd_amd_decode_batch_geometry) is three planes in one block, the I422 convention: Y, H rows of W elements picture_pitch bytes apart, at
 * 0; Cb, H rows of W / 2 elements picture_pitch / 2 bytes apart, at H * picture_pitch; Cr, the same, at H * picture_pitch + H * picture_pitch / 2 -- always Y, Cb, Cr,
 * whatever the packed order (Cb is byte 1 of YUY2's Y0 U Y1 V, byte 0 of 2vuy's U Y0 V Y1, word 3 of YU64's Y0 C1 Y1 C2; Cr byte 3, byte 2, word 1); interlaced
 * pictures keep their frame rows.  A contiguous picture is picture_pitch = W * element size and occupies 2 * H * picture_pitch bytes: one row of a torch tensor
 * (n, 2 * H * W) views as Y (H, W) and CbCr (2, H, W / 2).  _U8 exists for YUY2 and 2vuy only, _U16 for YU64 only: the byte or word as it is.  _F32: (float)w *
 * (1.0f / unit) with the unit of the batch's own word, 255 or 65535, one IEEE single multiply; _F16: that value rounded to nearest-even to binary16, subnormals
 * kept.  No range scaling and no chroma offset: 0.5 is roughly neutral chroma.  CFHD_AMD_FRAMES_YUV422_* of cfhd_amd_batch_upload_device_planar invert these rules:
 * for the 8-bit unit collect(deliver(b)) = b for all 256 bytes through U8, F32 and also F16; for the 16-bit unit U16 and F32 are exact for all 65 536 words and F16
 * is idempotent.  The pitch is a multiple of 32 (the chroma pitch: of 16) and >= W * element size; the stride is >= H * picture_pitch + (2 H - 1) * (picture_pitch / 2)
 * + the chroma row bytes.  Written by k_dec_deliver_yuv422 in place of k_dec_deliver (kernel_name(batch, 9) answers it while such a layout is set; kernel_ms index 9
 * times it).
 * CFHD_AMD_PICTURES_RGBA_U8 / _U16 / _F16 / _F32: every batch whose output is b64a, BGRA or BGRa -- intra batches of 4:2:2, RGB 4:4:4 and RGBA 4:4:4:4 samples and group
 * batches, at full and half resolution where the batch serves it -- and no other (to every other batch the values are unknown layouts).  The picture of W x H pixels
 * (cfhd_amd_decode_batch_geometry) is four planes, R, then G, then B, then A, each H rows of W elements, rows picture_pitch bytes apart, planes H * picture_pitch
 * apart: a contiguous tensor (n, 4, H, W) is picture_pitch = W * element size, picture_stride = 4 * H * picture_pitch.  The plane order is always R, G, B, A,
 * whatever the packed order (b64a: the native 16-bit words A, R, G, B; BGRA and BGRa: the bytes B, G, R, A), and the planes always have the top row first: plane row r
 * of a BGRA picture, whose packed form has the bottom row first, is packed row H - 1 - r; BGRa and b64a keep their order; interlaced pictures keep their frame rows.
 * _U8 exists for BGRA and BGRa only, _U16 for b64a only: the byte or word as it is.  _F32: (float)w * (1.0f / unit) with the unit of the batch's own word, 255 or
 * 65535, one IEEE single multiply; _F16: that value rounded to nearest-even to binary16, subnormals kept.  Alpha is a component like the others: the packed byte or
 * word, no companding, no premultiplication; the constant alpha of a picture whose sample had none arrives as it stands in the packed picture (b64a: 0xffff of 4:2:2,
 * 0xfff0 of RGB 4:4:4 samples; BGRA / BGRa: the byte the conversion writes).  CFHD_AMD_FRAMES_RGBA_* of cfhd_amd_batch_upload_device_planar invert these rules as
 * the YUV422 layouts do.  The pitch is >= W * element size; the stride is >= (4 H - 1) * picture_pitch + W * element size.  Written by k_dec_deliver_rgba in place
 * of k_dec_deliver (kernel_name(batch, 9) answers it while such a layout is set; kernel_ms index 9 times it).
 * CFHD_AMD_PICTURES_RGB_AS_YU64 / _RGB_AS_YUV422_U16 / _F16 / _F32: the YU64 picture of an RGB sample, for the consumer that holds an RGB master and needs 4:2:2 -- served
 * on a batch made by cfhd_amd_decode_batch_create from an RGB 4:4:4 or RGBA 4:4:4:4 sample with output RG48 at full resolution, whose width is even; every other
 * batch whose output is RG48 (a 4:2:2 sample -- it decodes to YU64 directly --, a batch of groups, half resolution) is told so, and to every batch with another output
 * the values are unknown layouts.  (CFHD_PrepareToDecode and cfhd_amd_decode_batch_create keep refusing YU64 of such a sample: the conversion lives in the delivery.)
 * The values are those the reference decoder writes for the same sample and output YU64, word for word: a pure function of the batch's RG48 picture r, g, b (0 ..
 * 65535).  Pixels (2 k, 2 k + 1) of a row form a pair; with every product and sum an IEEE single of its own (never fused), evaluated as (cr * R + cg * G) + cb * B,
 * every coefficient (float)c * 64.0f, the conversion to int truncating toward zero and >> arithmetic:
 *   Y(x)  = sat16(((int)(yr r + yg g + yb b) >> 6) + 4096)
 *   Cb(k) = sat16(((int)(ur (r0 + r1) + ug (g0 + g1) + ub (b0 + b1)) >> 7) + 32768); Cr(k) the same with the v row; the sums are converted to single once;
 * sat16 clamps to 0 .. 65535.  The rows (y; u; v) are (0.183, 0.614, 0.062; -0.101, -0.338, 0.439; 0.439, -0.399, -0.040) for a sample without a colour-space tag
 * or with bit 2 (value 4) of it clear, and (0.213, 0.715, 0.072; -0.117, -0.394, 0.511; 0.511, -0.464, -0.047) with the bit set; 4096 is added under both, so bright
 * pixels saturate under the second: the reference's behaviour.  Every picture is converted with the matrix of its own sample's tag; a pass may mix them (a sample whose
 * tag differs from the first sample's is decoded by the handle inside wait and delivered by a launch of its own there).  The picture of a sample that failed is
 * zeros (0.0), not the conversion of black.
 * _RGB_AS_YU64: the packed picture, rows of 4 * W bytes, the words Y0 Cr Y1 Cb; the pitch is a multiple of 16 and >= 4 * W, the stride >= (H - 1) * picture_pitch
 * + 4 * W.  _RGB_AS_YUV422_U16 / _F16 / _F32: the same words as three planes in exactly the geometry of CFHD_AMD_PICTURES_YUV422_* (Y: H rows of W elements; Cb, Cr:
 * H rows of W / 2 elements at half the pitch; the pitch a multiple of 32, the stride rule that of the YUV422 layouts), _F32 (float)w * (1.0f / 65535.0f), _F16 that
 * value rounded to nearest-even to binary16.  Written by k_dec_deliver_rgb_as_yuv in place of k_dec_deliver (kernel_name(batch, 9) answers it while such a layout is
 * set; kernel_ms index 9 times it).  Host delivery and cfhd_amd_decode_batch_download_output give the RG48 picture beside it, unchanged.
 * CFHD_AMD_PICTURES_RGB10_U16 / _F16 / _F32: a batch made by cfhd_amd_decode_batch_create_thumbnails only (to every other batch the values are unknown layouts; on such
 * a batch every layout but these and PACKED is refused).  The picture of W8 x H8 DPX0 words is three planes, R, then G, then B, each H8 rows of W8 elements, rows
 * picture_pitch bytes apart, planes H8 * picture_pitch apart: a contiguous tensor (n, 3, H8, W8) is picture_pitch = W8 * element size, picture_stride = 3 * H8 *
 * picture_pitch.  _U16: the 10-bit value as it is, 0 .. 1023; _F32: (float)v * (1.0f / 1023.0f), one IEEE single multiply; _F16: that value rounded to nearest-even to
 * binary16.  The pitch is >= W8 * element size; the stride is >= (3 H8 - 1) * picture_pitch + W8 * element size.  Written by k_dec_deliver_rgb10 in place of
 * k_dec_deliver (kernel_name(batch, 9) answers it while such a layout is set; kernel_ms index 9 times it).
 * Exactly count pictures are written, of every row its row bytes and nothing else: pitch padding, the space between planes and pictures and the pictures behind a short
 * pass are not touched.
 * 0; -1 with the reason in cfhd_amd_last_error(): a pass in flight, an unknown layout, a planar layout on a batch whose output is not RG48, a pointer, stride or pitch
 * that is no multiple of 16, a pitch below the row bytes of the layout, a stride below what one picture occupies; a 4:2:2 plane layout on a batch whose output is not
 * YUY2, 2vuy or YU64, _U8 on a YU64 batch, _U16 on an 8-bit one, a pitch of such a layout that is no multiple of 32; RGBA_U8 on a b64a batch, RGBA_U16 on a BGRA or
 * BGRa one; an RGB_AS_* layout on an RG48 batch it does not serve, on an odd width, with a pitch below its row (or, the plane forms, no multiple of 32), with a
 * stride below its rows or planes; on a thumbnail batch any layout but PACKED and RGB10_*, an RGB10 pitch below its plane row, a stride below its three planes. */
enum { CFHD_AMD_PICTURES_PACKED = 0, CFHD_AMD_PICTURES_PLANAR_U16 = 1, CFHD_AMD_PICTURES_PLANAR_F16 = 2, CFHD_AMD_PICTURES_PLANAR_F32 = 3 };
enum { CFHD_AMD_PICTURES_BAYER_U16 = 4, CFHD_AMD_PICTURES_BAYER_F16 = 5, CFHD_AMD_PICTURES_BAYER_F32 = 6 };
enum { CFHD_AMD_PICTURES_YUV422_U8 = 7, CFHD_AMD_PICTURES_YUV422_U16 = 8, CFHD_AMD_PICTURES_YUV422_F16 = 9, CFHD_AMD_PICTURES_YUV422_F32 = 10 };
enum { CFHD_AMD_PICTURES_RGBA_U8 = 11, CFHD_AMD_PICTURES_RGBA_U16 = 12, CFHD_AMD_PICTURES_RGBA_F16 = 13, CFHD_AMD_PICTURES_RGBA_F32 = 14 };
enum { CFHD_AMD_PICTURES_RGB_AS_YU64 = 15, CFHD_AMD_PICTURES_RGB_AS_YUV422_U16 = 16, CFHD_AMD_PICTURES_RGB_AS_YUV422_F16 = 17, CFHD_AMD_PICTURES_RGB_AS_YUV422_F32 = 18 };
enum { CFHD_AMD_PICTURES_RGB10_U16 = 19, CFHD_AMD_PICTURES_RGB10_F16 = 20, CFHD_AMD_PICTURES_RGB10_F32 = 21 };
int  cfhd_amd_decode_batch_set_device_pictures(cfhd_amd_decode_batch *batch, void *d_pictures, size_t picture_stride, int picture_pitch, int layout);
/* Collects the pass: the number of samples that decoded, or < 0 (-1: nothing in flight, -2: device failure).  status (NULL or count entries): status[i] is the CFHD_Error
 * CFHD_DecodeSample returns for sample i on a handle prepared on the first sample; the picture of a sample that failed is zero.  Samples the device parser refuses are
 * final there; samples the device stage does not place (longer than width x height x bytes per pixel + 64 KB, a size that is no multiple of 4), samples whose scan or
 * colour-space tag differs from the first sample's and -- when any code stream of the pass is damaged -- every sample the parser passed are decoded by that handle
 * inside this call. */
int  cfhd_amd_decode_batch_wait(cfhd_amd_decode_batch *batch, CFHD_Error *status);
/* Picture i of the last pass into out (rows `pitch` >= row_bytes apart): from HBM, or, for a sample the handle decoded inside wait, the handle's picture, which the
 * batch keeps whichever way the pass delivered its pictures -- what this call gives always agrees with status[i].  0, -1 for bad arguments or a pass in flight, -2 for a device failure. */
int  cfhd_amd_decode_batch_download_output(cfhd_amd_decode_batch *batch, int i, void *out, int pitch);
/* HIP-event time (ms) of the kernels of the last pass and their names as a profiler shows them.  which: 0 k_dec_ingest, 1 k_dec_parse, 2 the band decoder (all its
 * kernels), 3 k_dec_lowpass, 4 / 5 / 6 the transform levels in launch order (the last one with the output conversion), 7 k_dec_blank, 9 k_dec_deliver (both kinds of
 * batch; k_dec_deliver_bayer while a BAYER_* layout is set, k_dec_deliver_yuv422 while a YUV422_* one is, k_dec_deliver_rgba while an RGBA_* one is, k_dec_deliver_rgb_as_yuv while an RGB_AS_* one is; a thumbnail batch: see cfhd_amd_decode_batch_create_thumbnails; 0 ms when the last pass delivered nothing into device memory).  0 / "" otherwise. */
float cfhd_amd_decode_batch_kernel_ms(cfhd_amd_decode_batch *batch, int which);
const char *cfhd_amd_decode_batch_kernel_name(cfhd_amd_decode_batch *batch, int which);
int  cfhd_amd_device_count(void);
/* Text of the last HIP / device failure behind a CFHD_ERROR_INTERNAL (the library has no CPU fallback: without a gfx950 device every
 * compute call fails and says why here). */
const char *cfhd_amd_last_error(void);
/* Fixes the otherwise random clip GUID that every new encoder stamps into its samples (16 bytes), for bit-exact diffs. */
void cfhd_amd_set_clip_guid(const unsigned char guid[16]);
/* Optional: page-lock a frame / output buffer the caller reuses, so that CFHD_EncodeSample, the encoder pool and CFHD_DecodeSample
 * move it over PCIe without a staging copy.  The caller keeps it alive and unregisters it before freeing it.  Returns 0 on success. */
int  cfhd_amd_register_host_buffer(void *buffer, size_t bytes);
int  cfhd_amd_unregister_host_buffer(void *buffer);

#ifdef __cplusplus
}
#endif
#endif
