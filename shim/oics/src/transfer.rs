//! `oics::transfer` (reference: packages/lib/src/transfer.rs) over the C ABI.
//! File decode / encode / windows stay host-side OpenCV calls; every pixel operation the corrector's
//! paths use (gray, threshold, resize, rotate, projections, the projection pictures) runs on the GPU.
use crate::bridge::{border_bytes, check, into_mat, view};
use crate::ffi;
use crate::types::{ImageFormat, RotateClipStrategy};
use opencv::core::{Mat, Scalar, Vector};
use opencv::prelude::*;
use opencv::{highgui, imgcodecs};

/// Owning wrapper over a `Mat` (transfer.rs:16-18).
pub struct TransformableMatrix {
    matrix: Mat,
}

// the reference asserts this too (transfer.rs:279); the wrapped Mat is only read concurrently
unsafe impl Sync for TransformableMatrix {}

impl TransformableMatrix {
    pub fn default() -> Self {
        TransformableMatrix { matrix: Mat::default() }
    }

    pub fn load_mat(self: &mut Self, filename: &str, flags: i32) -> Result<&mut Self, opencv::Error> {
        self.matrix = imgcodecs::imread(filename, flags)?;
        Ok(self)
    }

    pub fn get_mat(self: &Self) -> &Mat {
        &self.matrix
    }

    pub fn from_matrix(mat: &Mat) -> Self {
        TransformableMatrix { matrix: mat.clone() }
    }

    pub fn new(filename: &str, flags: i32) -> Result<Self, opencv::Error> {
        Ok(TransformableMatrix { matrix: imgcodecs::imread(filename, flags)? })
    }

    /// transfer.rs:66-91 -> omr_scale (INTER_LINEAR when enlarging, INTER_AREA otherwise).
    pub fn scale_self(self: &mut Self, scale: f64) -> Result<&mut Self, opencv::Error> {
        if scale == 1.0 {
            return Ok(self);
        }
        let mut out = ffi::OmrImageOwned::empty();
        check(unsafe { ffi::omr_scale(&view(&self.matrix)?, scale, &mut out) })?;
        self.matrix = into_mat(out)?;
        Ok(self)
    }

    /// transfer.rs:93-126 -> omr_shrink_to (never enlarges).
    pub fn shrink_to(self: &mut Self, max_width: i32, max_height: i32) -> Result<&mut Self, opencv::Error> {
        let mut out = ffi::OmrImageOwned::empty();
        check(unsafe { ffi::omr_shrink_to(&view(&self.matrix)?, max_width, max_height, &mut out) })?;
        self.matrix = into_mat(out)?;
        Ok(self)
    }

    /// transfer.rs:128-145 -> omr_resize (INTER_AREA).
    pub fn resize_self(self: &mut Self, width: i32, height: i32) -> Result<&mut Self, opencv::Error> {
        let mut out = ffi::OmrImageOwned::empty();
        check(unsafe { ffi::omr_resize(&view(&self.matrix)?, width, height, &mut out) })?;
        self.matrix = into_mat(out)?;
        Ok(self)
    }

    pub fn show(self: &Self, win_name: &str) -> Result<(), opencv::Error> {
        highgui::named_window(win_name, highgui::WINDOW_NORMAL)?;
        highgui::imshow(win_name, &self.matrix)
    }

    pub fn get_bytes(self: &Self) -> Result<&[u8], opencv::Error> {
        self.matrix.data_bytes()
    }

    pub fn im_write(self: &Self, filename: &str, format: ImageFormat, quality: i32) -> Result<bool, opencv::Error> {
        let key = match format {
            ImageFormat::JPEG => imgcodecs::IMWRITE_JPEG_QUALITY,
            ImageFormat::PNG => imgcodecs::IMWRITE_PNG_COMPRESSION,
            ImageFormat::WEBP => imgcodecs::IMWRITE_WEBP_QUALITY,
        };
        let params: Vector<i32> = Vector::from_slice(&[key, quality]);
        imgcodecs::imwrite(filename, &self.matrix, &params)
    }

    pub fn clone(&self) -> Self {
        TransformableMatrix { matrix: self.matrix.clone() }
    }

    /// transfer.rs:206-231 -> omr_morph (OMR_MORPH_DILATE): getStructuringElement(kernel_shape, kernel_size, anchor),
    /// `iterations` passes, BORDER_CONSTANT with the default border value, any channel count, on the GPU.
    pub fn dilate(&self, kernel_shape: i32, kernel_size: opencv::core::Size, anchor: opencv::core::Point, iterations: i32) -> opencv::Result<Self> {
        let mut out = ffi::OmrImageOwned::empty();
        check(unsafe {
            ffi::omr_morph(&view(&self.matrix)?, 1, kernel_shape, kernel_size.width, kernel_size.height, anchor.x, anchor.y, iterations, &mut out)
        })?;
        Ok(TransformableMatrix { matrix: into_mat(out)? })
    }

    /// transfer.rs:254-277 -> omr_morph (OMR_MORPH_ERODE).
    /// (The erode that IS on path 2, omr.rs:98-112, runs inside omr_get_result_from_projection.)
    pub fn erode(&self, kernel_shape: i32, kernel_size: opencv::core::Size, anchor: opencv::core::Point, iterations: i32) -> opencv::Result<Self> {
        let mut out = ffi::OmrImageOwned::empty();
        check(unsafe {
            ffi::omr_morph(&view(&self.matrix)?, 0, kernel_shape, kernel_size.width, kernel_size.height, anchor.x, anchor.y, iterations, &mut out)
        })?;
        Ok(TransformableMatrix { matrix: into_mat(out)? })
    }
}

fn new_u8c1(rows: i32, cols: i32) -> opencv::Result<Mat> {
    Mat::new_rows_cols_with_default(rows, cols, opencv::core::CV_8UC1, Scalar::all(0.0))
}

/// transfer.rs:283-290: cvtColor(RGB2GRAY) -> omr_rgb_to_gray.
pub fn transfer_rgb_image_to_gray_image(src: &TransformableMatrix) -> Result<TransformableMatrix, opencv::Error> {
    let v = view(&src.matrix)?;
    let mut dst = new_u8c1(v.rows, v.cols)?;
    let step = dst.step1(0)? as i64;
    check(unsafe { ffi::omr_rgb_to_gray(&v, dst.data_mut(), step) })?;
    Ok(TransformableMatrix { matrix: dst })
}

/// `transfer_rgb_image_to_gray_image` for `n` same-shape scans of 3 or 4 channels that already live in device memory
/// (omr_rgb_to_gray_batch_device): scan i at `d_src + i * src_stride_bytes`, its gray image at `d_dst + i *
/// dst_stride_bytes`, one launch, enqueued on `stream` (a hipStream_t, null for the default one).  Byte for byte the
/// per-image conversion.  Not in the reference crate.
///
/// # Safety
/// `d_src` and `d_dst` are device pointers that span the strides and steps given.
pub unsafe fn rgb_images_to_gray(
    d_src: *const u8,
    n: i32,
    src_stride_bytes: i64,
    src_step: i64,
    rows: i32,
    cols: i32,
    channels: i32,
    d_dst: *mut u8,
    dst_stride_bytes: i64,
    dst_step: i64,
    stream: *mut std::os::raw::c_void,
) -> opencv::Result<()> {
    check(ffi::omr_rgb_to_gray_batch_device(d_src, n, src_stride_bytes, src_step, rows, cols, channels, d_dst, dst_stride_bytes, dst_step, stream))
}

/// transfer.rs:294-301: threshold(127, 255, BINARY) -> omr_threshold_binary.
pub fn transfer_gray_image_to_thresh_binary(src: &TransformableMatrix) -> Result<TransformableMatrix, opencv::Error> {
    let v = view(&src.matrix)?;
    let mut dst = new_u8c1(v.rows, v.cols)?;
    let step = dst.step1(0)? as i64;
    check(unsafe { ffi::omr_threshold_binary(&v, dst.data_mut(), step) })?;
    Ok(TransformableMatrix { matrix: dst })
}

/// transfer.rs:305-333: black pixels per row.
pub fn get_horizontal_projection(src: &TransformableMatrix) -> Result<Vec<f64>, opencv::Error> {
    let v = view(&src.matrix)?;
    let mut out = vec![0.0f64; v.rows as usize];
    check(unsafe { ffi::omr_get_horizontal_projection(&v, out.as_mut_ptr()) })?;
    Ok(out)
}

/// transfer.rs:380-405: black pixels per column.
pub fn get_vertical_projection(src: &TransformableMatrix) -> Result<Vec<f64>, opencv::Error> {
    let v = view(&src.matrix)?;
    let mut out = vec![0.0f64; v.cols as usize];
    check(unsafe { ffi::omr_get_vertical_projection(&v, out.as_mut_ptr()) })?;
    Ok(out)
}

/// transfer.rs:337-376 -> omr_projection_pictures (horizontal).  Any 8-bit values: per row the pixels before the first
/// `== 255` stay as they are, then come as many 0 as the row has pixels `!= 255` in all, then 255.
pub fn transfer_thresh_binary_to_horizontal_projection(src: &TransformableMatrix) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_projection_pictures(&view(&src.matrix)?, &mut out, std::ptr::null_mut()) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// transfer.rs:409-455 -> omr_projection_pictures (vertical).  Any 8-bit values: column c gets a black bar from the
/// bottom edge as high as the column has pixels `<= 127`; the rest is 255.
pub fn transfer_thresh_binary_to_vertical_projection(src: &TransformableMatrix) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_projection_pictures(&view(&src.matrix)?, std::ptr::null_mut(), &mut out) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// transfer.rs:459-523 -> omr_rotate_ex.  `flags` and `border_mode` go to warpAffine as the reference passes them:
/// INTER_NEAREST (0, the numeric value of WARP_POLAR_LINEAR), LINEAR, CUBIC, AREA (= LINEAR) or LANCZOS4, with
/// WARP_INVERSE_MAP / WARP_FILL_OUTLIERS; BORDER_CONSTANT .. BORDER_TRANSPARENT.  Flags 5..7 are OMR_ERR_NOTIMPL.
pub fn rotate_mat(
    src: &TransformableMatrix,
    angle: f64,
    scale: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
) -> Result<TransformableMatrix, opencv::Error> {
    let border = border_bytes(border_value);
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe {
        ffi::omr_rotate_ex(&view(&src.matrix)?, angle, scale, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), &mut out)
    })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// `rotate_mat` for a slice of images with an angle each -> omr_rotate_batch_ex: one call for the whole slice (images of
/// one shape share an upload of their matrices and a launch), the results in the order of `srcs`, each what
/// `rotate_mat(&srcs[i], angles[i], ..)` returns.  Scale, flags, border and clip strategy are the batch's.
pub fn rotate_mats(
    srcs: &[TransformableMatrix],
    angles: &[f64],
    scale: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
) -> Result<Vec<TransformableMatrix>, opencv::Error> {
    if srcs.len() != angles.len() {
        return Err(opencv::Error::new(ffi::OMR_ERR_BADARG, String::from("rotate_mats: one angle per image")));
    }
    let border = border_bytes(border_value);
    let mut views = Vec::with_capacity(srcs.len());
    for s in srcs {
        views.push(view(&s.matrix)?);
    }
    let mut outs: Vec<ffi::OmrImageOwned> = (0..srcs.len()).map(|_| ffi::OmrImageOwned::empty()).collect();
    check(unsafe {
        ffi::omr_rotate_batch_ex(views.as_ptr(), srcs.len() as i32, angles.as_ptr(), scale, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), outs.as_mut_ptr())
    })?;
    // every image is taken over before the first error is reported, so none of the library's buffers is lost
    let mats: Vec<opencv::Result<Mat>> = outs.into_iter().map(into_mat).collect();
    mats.into_iter().map(|m| Ok(TransformableMatrix { matrix: m? })).collect()
}

/// transfer.rs:527-536 -> (std-dev of the vertical projection, std-dev of the horizontal projection).
pub fn get_projection_standard_deviations(src: &TransformableMatrix) -> Result<(f64, f64), opencv::Error> {
    let (mut v_sd, mut h_sd) = (0.0f64, 0.0f64);
    check(unsafe { ffi::omr_get_projection_standard_deviations(&view(&src.matrix)?, &mut v_sd, &mut h_sd) })?;
    Ok((v_sd, h_sd))
}

/// The bytes `im_write(.., ImageFormat::JPEG, quality)` puts into its file, encoded on the GPU (omr_jpeg_encode): what
/// libjpeg writes for the Mat after jpeg_set_defaults + jpeg_set_quality.  Gray or BGR, 8-bit.  Not in the reference crate.
/// One call in the usual case: the first buffer holds the raw image's size plus the header; a stream that does not fit
/// (noise at the highest qualities) answers OMR_ERR_NOMEM with its length, and a second call encodes again into that.
pub fn encode_jpeg(m: &TransformableMatrix, quality: i32) -> Result<Vec<u8>, opencv::Error> {
    let v = view(&m.matrix)?;
    let mut bound = 0i64;
    check(unsafe { ffi::omr_jpeg_bound(v.rows, v.cols, v.channels, &mut bound) })?;
    let raw = v.rows as i64 * v.cols as i64 * v.channels as i64 + 1024;
    let mut out = vec![0u8; raw.min(bound) as usize];
    let mut len = 0i64;
    let mut rc = unsafe { ffi::omr_jpeg_encode(&v, quality, out.as_mut_ptr(), out.len() as i64, &mut len) };
    if rc == ffi::OMR_ERR_NOMEM {
        out = vec![0u8; len as usize];
        rc = unsafe { ffi::omr_jpeg_encode(&v, quality, out.as_mut_ptr(), out.len() as i64, &mut len) };
    }
    check(rc)?;
    out.truncate(len as usize);
    Ok(out)
}

/// A PNG stream that decodes to the Mat exactly, encoded on the GPU (omr_png_encode): what `im_write(.., ImageFormat::PNG,
/// level)` is for, lossless and deterministic, but not imwrite's bytes (PNG has no canonical stream).  Gray, BGR or BGRA,
/// 8-bit; `compression` is IMWRITE_PNG_COMPRESSION: 0 stores, 1 .. 9 all compress alike.  Not in the reference crate.
/// One call in the usual case: the first buffer holds half the raw image's size; a stream that does not fit answers
/// OMR_ERR_NOMEM with its length, and a second call encodes again into that.
pub fn encode_png(m: &TransformableMatrix, compression: i32) -> Result<Vec<u8>, opencv::Error> {
    let v = view(&m.matrix)?;
    let mut bound = 0i64;
    check(unsafe { ffi::omr_png_bound(v.rows, v.cols, v.channels, &mut bound) })?;
    let raw = v.rows as i64 * v.cols as i64 * v.channels as i64 / 2 + 1024;
    let mut out = vec![0u8; raw.min(bound) as usize];
    let mut len = 0i64;
    let mut rc = unsafe { ffi::omr_png_encode(&v, compression, out.as_mut_ptr(), out.len() as i64, &mut len) };
    if rc == ffi::OMR_ERR_NOMEM {
        out = vec![0u8; len as usize];
        rc = unsafe { ffi::omr_png_encode(&v, compression, out.as_mut_ptr(), out.len() as i64, &mut len) };
    }
    check(rc)?;
    out.truncate(len as usize);
    Ok(out)
}

/// A CCITT Group 4 TIFF file of the Mat thresholded at `threshold` (0 .. 254; a pixel is white iff its gray value is
/// above it), encoded on the GPU (omr_tiff_encode): gray or BGR, 8-bit.  The strips are byte for byte what libtiff writes
/// for that picture.  `rows_per_strip` 0: one strip; `dpi` 0: no resolution tags.  Not in the reference crate.
pub fn encode_tiff(m: &TransformableMatrix, threshold: i32, rows_per_strip: i32, dpi: i32) -> Result<Vec<u8>, opencv::Error> {
    let v = view(&m.matrix)?;
    let mut bound = 0i64;
    check(unsafe { ffi::omr_tiff_bound(v.rows, v.cols, rows_per_strip, &mut bound) })?;
    let first = v.rows as i64 * v.cols as i64 / 8 + 4096;
    let mut out = vec![0u8; first.min(bound) as usize];
    let mut len = 0i64;
    let mut rc = unsafe { ffi::omr_tiff_encode(&v, threshold, rows_per_strip, dpi, out.as_mut_ptr(), out.len() as i64, &mut len) };
    if rc == ffi::OMR_ERR_NOMEM {
        out = vec![0u8; len as usize];
        rc = unsafe { ffi::omr_tiff_encode(&v, threshold, rows_per_strip, dpi, out.as_mut_ptr(), out.len() as i64, &mut len) };
    }
    check(rc)?;
    out.truncate(len as usize);
    Ok(out)
}

/// An 8-bit TIFF file of the Mat, gray or RGB, encoded on the GPU (omr_tiff8_encode): `compression` 1 (none) or 5 (LZW),
/// `predictor` 1, or 2 with LZW.  The file decodes to the Mat exactly.  `rows_per_strip` 0: libtiff's default, strips of
/// at most 8192 raw bytes; `dpi` 0: no resolution tags.  Not in the reference crate.
pub fn encode_tiff8(m: &TransformableMatrix, compression: i32, predictor: i32, rows_per_strip: i32, dpi: i32) -> Result<Vec<u8>, opencv::Error> {
    let v = view(&m.matrix)?;
    let mut bound = 0i64;
    check(unsafe { ffi::omr_tiff8_bound(v.rows, v.cols, v.channels, compression, rows_per_strip, &mut bound) })?;
    let first = v.rows as i64 * v.cols as i64 * v.channels as i64 + 8 * v.rows as i64 + 4096;
    let mut out = vec![0u8; first.min(bound) as usize];
    let mut len = 0i64;
    let mut rc = unsafe { ffi::omr_tiff8_encode(&v, compression, predictor, rows_per_strip, dpi, out.as_mut_ptr(), out.len() as i64, &mut len) };
    if rc == ffi::OMR_ERR_NOMEM {
        out = vec![0u8; len as usize];
        rc = unsafe { ffi::omr_tiff8_encode(&v, compression, predictor, rows_per_strip, dpi, out.as_mut_ptr(), out.len() as i64, &mut len) };
    }
    check(rc)?;
    out.truncate(len as usize);
    Ok(out)
}

/// What `im_read` gives for a file with these bytes (`imread(.., IMREAD_COLOR)` for `channels` = 3, `IMREAD_GRAYSCALE`
/// for 1), decoded on the GPU (omr_jpeg_decode): libjpeg's output with its defaults, byte for byte.  Baseline streams;
/// one the decoder refuses (progressive, CMYK, an EXIF orientation, ..) is an error with code OMR_ERR_NOTIMPL, so that
/// the caller can hand the file to its host codec.  Not in the reference crate.
pub fn decode_jpeg(stream: &[u8], channels: i32) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_jpeg_decode(stream.as_ptr(), stream.len() as i64, channels, &mut out) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// What `im_read` gives for a PNG file with these bytes (`imread(.., IMREAD_COLOR)` for `channels` = 3,
/// `IMREAD_GRAYSCALE` for 1), decoded on the GPU (omr_png_decode): libpng's rows after OpenCV's transforms, byte for byte.
/// Non-interlaced streams of 8 bits or fewer; one the decoder refuses (Adam7, 16-bit, gray from a colour stream, an EXIF
/// orientation, APNG) is an error with code OMR_ERR_NOTIMPL, so that the caller can hand the file to its host codec.  Not
/// in the reference crate.
pub fn decode_png(stream: &[u8], channels: i32) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_png_decode(stream.as_ptr(), stream.len() as i64, channels, &mut out) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// What `im_read` gives for a TIFF file with these bytes, decoded on the GPU (omr_tiff_decode): libtiff's rows, byte for
/// byte.  1-bit strips (uncompressed, PackBits or CCITT Group 4) as 255 / 0; 8-bit gray and RGB strips (uncompressed,
/// PackBits or LZW, Predictor 1 or 2), an RGB file as BGR.  One the decoder refuses (BigTIFF, tiles, other depths or
/// compressions, palette, alpha, an Orientation tag, a gray image asked of an RGB file) is an error with code
/// OMR_ERR_NOTIMPL, so that the caller can hand the file to its host codec.  Not in the reference crate.
pub fn decode_tiff(stream: &[u8], channels: i32) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_tiff_decode(stream.as_ptr(), stream.len() as i64, channels, &mut out) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// An image turned by an EXIF orientation code 1..8 (omr_orient), on the GPU: what `imread` does to a JPEG that carries
/// one (OpenCV's ExifTransform).  Gray or BGR, 8-bit.  Not in the reference crate.
pub fn orient(m: &TransformableMatrix, orientation: i32) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_orient(&view(&m.matrix)?, orientation, &mut out) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}

/// What `im_read` gives for a file with these bytes, JPEG, PNG or bilevel TIFF (told apart by PNG's signature and TIFF's
/// byte-order mark), decoded on the GPU (omr_imread): `decode_jpeg` / `decode_png` / `decode_tiff`, and a JPEG with an EXIF orientation 2..8 is turned as `imread` turns it.
/// `flags`: 0, or `ImReadFlags::from(ImReadFlags::IgnoreOrientation)` (= `ffi::OMR_IMREAD_IGNORE_ORIENTATION`) to decode
/// as stored.  Not in the reference crate.
pub fn imread(stream: &[u8], channels: i32, flags: i32) -> Result<TransformableMatrix, opencv::Error> {
    let mut out = ffi::OmrImageOwned::empty();
    check(unsafe { ffi::omr_imread(stream.as_ptr(), stream.len() as i64, channels, flags, &mut out) })?;
    Ok(TransformableMatrix { matrix: into_mat(out)? })
}
