//! `oics::fft` (reference: packages/lib/src/fft.rs) -> omr_get_fft_image / omr_get_angle_with_fft / _ex,
//! and the batch form omr_get_angles_with_fft_batch.
use crate::bridge::{border_bytes, check, into_mat, view};
use crate::ffi;
use crate::projection::files_through;
use crate::transfer::TransformableMatrix;
use crate::types::RotateClipStrategy;
use opencv::core::{Mat, Scalar, Vector};
use opencv::imgcodecs;
use opencv::prelude::*;
use std::path::Path;

/// fft.rs:32: 1 - filter, element-wise (float Mat helper of the reference's filter experiments; host OpenCV).
pub fn rev(filter: &Mat) -> opencv::Result<Mat> {
    let mut neg = Mat::default();
    filter.convert_to(&mut neg, -1, -1.0, 1.0)?; // -1 * x + 1
    Ok(neg)
}

/// fft.rs:124-141 -> (magnitude_image, magnitude_log_image), both 8-bit single channel.
pub fn get_fft_image(gray_tm: &TransformableMatrix) -> opencv::Result<(Mat, Mat)> {
    let (mut mag, mut mag_log) = (ffi::OmrImageOwned::empty(), ffi::OmrImageOwned::empty());
    check(unsafe { ffi::omr_get_fft_image(&view(gray_tm.get_mat())?, &mut mag, &mut mag_log) })?;
    let m = into_mat(mag);
    let l = into_mat(mag_log);
    Ok((m?, l?))
}

/// fft.rs:145-256: spectrum picture -> Canny(t1, t2) -> HoughLinesP(threshold 100) -> the reference's vote
/// (including its fft.rs:231 quirk), all on the GPU.  The debug picture (fft.rs:173-213, :248-253: the edges of
/// the log spectrum in colour with every segment drawn on) comes from omr_get_angle_with_fft_ex in the same pass and
/// is written when `edge_image_output_dir` is not empty.
pub fn get_angle_with_fft(
    gray_tm: &TransformableMatrix,
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
    file_name: &str,
    edge_image_output_dir: &str,
) -> Result<f64, opencv::Error> {
    let v = view(gray_tm.get_mat())?;
    let mut angle = 0.0f64;
    if edge_image_output_dir.is_empty() {
        check(unsafe { ffi::omr_get_angle_with_fft(&v, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, &mut angle) })?;
    } else {
        let mut lined = ffi::OmrImageOwned::empty();
        check(unsafe {
            ffi::omr_get_angle_with_fft_ex(&v, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, &mut angle, &mut lined)
        })?;
        let pic = into_mat(lined)?;
        let path = Path::new(edge_image_output_dir).join(file_name);
        let params: Vector<i32> = Vector::from_slice(&[imgcodecs::IMWRITE_JPEG_QUALITY, 100]);
        imgcodecs::imwrite(path.to_str().unwrap_or(file_name), &pic, &params)?;
    }
    Ok(angle)
}

/// `get_angle_with_fft` for a batch: 8-bit single-channel images of any mix of shapes, one angle per image at the image's
/// own position, each the angle the per-call function returns (same f64 bits; 0.0 where no segment is found, as there).
/// Same-shape images go through the transform, Canny and HoughLinesP together on the device.  An invalid image fails
/// the whole batch.
pub fn get_angles_with_fft(
    grays: &[&TransformableMatrix],
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
) -> opencv::Result<Vec<f64>> {
    let n = grays.len();
    let views: Vec<ffi::OmrImage> = grays.iter().map(|g| view(g.get_mat())).collect::<opencv::Result<_>>()?;
    let mut angles = vec![0.0f64; n];
    check(unsafe {
        ffi::omr_get_angles_with_fft_batch(views.as_ptr(), n as i32, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, angles.as_mut_ptr(), std::ptr::null_mut())
    })?;
    Ok(angles)
}

/// The same with the picture `get_angle_with_fft` writes for every scan -- the edges of the log spectrum in colour with
/// every segment drawn on (fft.rs:173-213), the bare edges where there is none -- as a `Mat`; encoding and writing stay
/// with the caller.
pub fn get_angles_with_fft_with_pictures(
    grays: &[&TransformableMatrix],
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
) -> opencv::Result<Vec<(f64, Mat)>> {
    let n = grays.len();
    let views: Vec<ffi::OmrImage> = grays.iter().map(|g| view(g.get_mat())).collect::<opencv::Result<_>>()?;
    let mut angles = vec![0.0f64; n];
    let mut lined: Vec<ffi::OmrImageOwned> = (0..n).map(|_| ffi::OmrImageOwned::empty()).collect();
    check(unsafe {
        ffi::omr_get_angles_with_fft_batch(views.as_ptr(), n as i32, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, angles.as_mut_ptr(), lined.as_mut_ptr())
    })?;
    // every picture is taken over (and so released) even when an earlier one fails to convert
    let mats: Vec<opencv::Result<Mat>> = lined.into_iter().map(into_mat).collect();
    mats.into_iter().enumerate().map(|(i, m)| Ok((angles[i], m?))).collect()
}

/// The FFT leg of the reference's benchmark (core/src/main.rs:133-170) for a batch: `get_angle_with_fft` on
/// `transfer_rgb_image_to_gray_image` of every image, then `rotate_mat` of the ORIGINAL by its angle
/// (omr_deskew_with_fft_batch).  Images of any mix of shapes, 1 or 3 channels each; result i belongs to image i: the
/// angle the per-call function returns (same f64 bits; 0.0 for a scan without a segment) with what `rotate_mat` gives
/// for it.  Not in the reference crate.
pub fn deskew_with_fft(
    srcs: &[&TransformableMatrix],
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
) -> opencv::Result<Vec<(f64, Mat)>> {
    let n = srcs.len();
    let views: Vec<ffi::OmrImage> = srcs.iter().map(|s| view(s.get_mat())).collect::<opencv::Result<_>>()?;
    let border = border_bytes(border_value);
    let mut angles = vec![0.0f64; n];
    let mut outs: Vec<ffi::OmrImageOwned> = (0..n).map(|_| ffi::OmrImageOwned::empty()).collect();
    check(unsafe {
        ffi::omr_deskew_with_fft_batch(views.as_ptr(), n as i32, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), angles.as_mut_ptr(), std::ptr::null_mut(), outs.as_mut_ptr())
    })?;
    // every image is taken over (and so released) even when an earlier one fails to convert
    let mats: Vec<opencv::Result<Mat>> = outs.into_iter().map(into_mat).collect();
    mats.into_iter().enumerate().map(|(i, m)| Ok((angles[i], m?))).collect()
}

/// The same from files to files (omr_deskew_with_fft_batch_streams): baseline JPEG or PNG files in, read as imread reads
/// them (an EXIF-tagged JPEG is turned), JPEG files at `quality` out, with nothing but file contents crossing to the GPU
/// and back.  Returns the angle per file.  A file its decoder refuses or cannot decode fails the call with that scan's
/// code and names it, and no output file is written.  Not in the reference crate.
pub fn deskew_files_with_fft(
    inputs: &[&str],
    outputs: &[&str],
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
    quality: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, jpeg, jpeg_len| unsafe {
        ffi::omr_deskew_with_fft_batch_streams(streams, len, n, 3, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), 0, quality, angles, scan_rc, jpeg, jpeg_len)
    })
}

/// `deskew_files_with_fft` with CCITT Group 4 TIFF files as its outputs (omr_deskew_with_fft_batch_streams_tiff): a pixel
/// is white iff its gray value is above `threshold` (0 .. 254); `rows_per_strip` 0: one strip a page; `dpi` 0: no
/// resolution tags.  Not in the reference crate.
pub fn deskew_files_with_fft_tiff(
    inputs: &[&str],
    outputs: &[&str],
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
    threshold: i32,
    rows_per_strip: i32,
    dpi: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, tiff, tiff_len| unsafe {
        ffi::omr_deskew_with_fft_batch_streams_tiff(streams, len, n, 3, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), threshold, rows_per_strip, dpi, angles, scan_rc, tiff, tiff_len)
    })
}

/// `deskew_files_with_fft` with 8-bit RGB TIFF files as its outputs (omr_deskew_with_fft_batch_streams_tiff8):
/// `compression` 1 (none) or 5 (LZW), `predictor` 1, or 2 with LZW; `rows_per_strip` 0: strips of at most 8192 raw bytes;
/// `dpi` 0: no resolution tags.  Not in the reference crate.
pub fn deskew_files_with_fft_tiff8(
    inputs: &[&str],
    outputs: &[&str],
    canny_threshold_1: f64,
    canny_threshold_2: f64,
    min_line_length: f64,
    max_line_gap: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
    compression: i32,
    predictor: i32,
    rows_per_strip: i32,
    dpi: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, tiff, tiff_len| unsafe {
        ffi::omr_deskew_with_fft_batch_streams_tiff8(streams, len, n, 3, canny_threshold_1, canny_threshold_2, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), compression, predictor, rows_per_strip, dpi, angles, scan_rc, tiff, tiff_len)
    })
}
