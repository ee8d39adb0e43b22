//! `oics::hough` (reference: packages/lib/src/hough.rs:17-100) -> omr_get_angle_with_hough / _ex,
//! and its batch form omr_get_angles_with_hough_batch.
use crate::bridge::{border_bytes, check, into_mat, view};
use crate::ffi;
use crate::projection::files_through;
use crate::transfer::TransformableMatrix;
use crate::types::RotateClipStrategy;
use opencv::core::{Mat, Scalar, Vector};
use opencv::imgcodecs;
use std::path::Path;

/// Canny(50, 150) -> HoughLinesP(1, pi/180, 0, min_line_length, max_line_gap) -> f32 atan2, `% 45`,
/// mode within 0.1 deg, all on the GPU.  The reference also writes a debug picture into `edge_image_output_dir`
/// (hough.rs:44-63, :91-96): the edge map in colour with every segment drawn on.  omr_get_angle_with_hough_ex
/// makes that picture in the same pass (Canny and HoughLinesP run once); encoding and writing it stay here, as
/// host-side codec work, and happen when the directory is not empty.
pub fn get_angle_with_hough(
    gray_tm: &TransformableMatrix,
    min_line_length: f64,
    max_line_gap: f64,
    file_name: &str,
    edge_image_output_dir: &str,
) -> Result<f64, opencv::Error> {
    let v = view(gray_tm.get_mat())?;
    let mut angle = 0.0f64;
    if edge_image_output_dir.is_empty() {
        check(unsafe { ffi::omr_get_angle_with_hough(&v, min_line_length, max_line_gap, &mut angle) })?;
    } else {
        let mut lined = ffi::OmrImageOwned::empty();
        check(unsafe { ffi::omr_get_angle_with_hough_ex(&v, min_line_length, max_line_gap, &mut angle, &mut lined) })?;
        let pic = into_mat(lined)?;
        let path = Path::new(edge_image_output_dir).join(file_name);
        let params: Vector<i32> = Vector::from_slice(&[imgcodecs::IMWRITE_JPEG_QUALITY, 100]);
        imgcodecs::imwrite(path.to_str().unwrap_or(file_name), &pic, &params)?;
    }
    Ok(angle)
}

/// What `get_angle_with_hough` answers for a scan in which HoughLinesP finds no segment (the reference panics on
/// `angles[0]`, hough.rs:74), for the scans of a batch: the batch call itself has succeeded.
fn scan_result(rc: i32, angle: f64) -> opencv::Result<f64> {
    if rc == ffi::OMR_OK {
        Ok(angle)
    } else {
        Err(opencv::Error::new(rc, String::from("no line segment found (the reference panics on angles[0], hough.rs:74)")))
    }
}

/// `get_angle_with_hough` for a batch: images of any mix of shapes and of 1, 3 or 4 channels, one result per image at
/// the image's own position, each the angle the per-call function returns (same f64 bits) or its error for a scan
/// without any segment.  Same-shape images go through Canny, HoughLinesP and the vote together on the device.  An
/// invalid image fails the whole batch: every entry then carries that error.
pub fn get_angles_with_hough(
    grays: &[&TransformableMatrix],
    min_line_length: f64,
    max_line_gap: f64,
) -> Vec<opencv::Result<f64>> {
    let n = grays.len();
    let views: opencv::Result<Vec<ffi::OmrImage>> = grays.iter().map(|g| view(g.get_mat())).collect();
    let views = match views {
        Ok(v) => v,
        Err(e) => return (0..n).map(|_| Err(opencv::Error::new(e.code, e.message.clone()))).collect(),
    };
    let mut angles = vec![0.0f64; n];
    let mut rc = vec![0i32; n];
    let call = check(unsafe {
        ffi::omr_get_angles_with_hough_batch(views.as_ptr(), n as i32, min_line_length, max_line_gap, angles.as_mut_ptr(), rc.as_mut_ptr(), std::ptr::null_mut())
    });
    if let Err(e) = call {
        return (0..n).map(|_| Err(opencv::Error::new(e.code, e.message.clone()))).collect();
    }
    (0..n).map(|i| scan_result(rc[i], angles[i])).collect()
}

/// The same with the picture `get_angle_with_hough` writes for every scan that has a result -- the edge map in colour
/// with every segment drawn on (hough.rs:44-63) -- as a `Mat`; encoding and writing stay with the caller.
pub fn get_angles_with_hough_with_pictures(
    grays: &[&TransformableMatrix],
    min_line_length: f64,
    max_line_gap: f64,
) -> Vec<opencv::Result<(f64, Mat)>> {
    let n = grays.len();
    let views: opencv::Result<Vec<ffi::OmrImage>> = grays.iter().map(|g| view(g.get_mat())).collect();
    let views = match views {
        Ok(v) => v,
        Err(e) => return (0..n).map(|_| Err(opencv::Error::new(e.code, e.message.clone()))).collect(),
    };
    let mut angles = vec![0.0f64; n];
    let mut rc = vec![0i32; n];
    let mut lined: Vec<ffi::OmrImageOwned> = (0..n).map(|_| ffi::OmrImageOwned::empty()).collect();
    let call = check(unsafe {
        ffi::omr_get_angles_with_hough_batch(views.as_ptr(), n as i32, min_line_length, max_line_gap, angles.as_mut_ptr(), rc.as_mut_ptr(), lined.as_mut_ptr())
    });
    if let Err(e) = call {
        return (0..n).map(|_| Err(opencv::Error::new(e.code, e.message.clone()))).collect();
    }
    lined
        .into_iter()
        .enumerate()
        .map(|(i, pic)| {
            let angle = scan_result(rc[i], angles[i])?;
            Ok((angle, into_mat(pic)?))
        })
        .collect()
}

/// The Hough leg of the reference's benchmark (core/src/main.rs:96-132) for a batch: `get_angle_with_hough` on
/// `transfer_rgb_image_to_gray_image` of every image, then `rotate_mat` of the ORIGINAL by its angle
/// (omr_deskew_with_hough_batch).  Images of any mix of shapes, 1 or 3 channels each; one result per image at the image's
/// own position: the angle the per-call function returns (same f64 bits) with what `rotate_mat` gives for it, or the
/// per-call error for a scan without any segment.  An invalid image fails the whole batch: every entry then carries
/// that error.  Not in the reference crate.
pub fn deskew_with_hough(
    srcs: &[&TransformableMatrix],
    min_line_length: f64,
    max_line_gap: f64,
    flags: i32,
    border_mode: i32,
    border_value: Scalar,
    clip_strategy: RotateClipStrategy,
) -> Vec<opencv::Result<(f64, Mat)>> {
    let n = srcs.len();
    let views: opencv::Result<Vec<ffi::OmrImage>> = srcs.iter().map(|s| view(s.get_mat())).collect();
    let views = match views {
        Ok(v) => v,
        Err(e) => return (0..n).map(|_| Err(opencv::Error::new(e.code, e.message.clone()))).collect(),
    };
    let border = border_bytes(border_value);
    let mut angles = vec![0.0f64; n];
    let mut rc = vec![0i32; n];
    let mut outs: Vec<ffi::OmrImageOwned> = (0..n).map(|_| ffi::OmrImageOwned::empty()).collect();
    let call = check(unsafe {
        ffi::omr_deskew_with_hough_batch(views.as_ptr(), n as i32, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), angles.as_mut_ptr(), rc.as_mut_ptr(), outs.as_mut_ptr())
    });
    if let Err(e) = call {
        return (0..n).map(|_| Err(opencv::Error::new(e.code, e.message.clone()))).collect();
    }
    outs.into_iter()
        .enumerate()
        .map(|(i, img)| {
            let angle = scan_result(rc[i], angles[i])?;
            Ok((angle, into_mat(img)?))
        })
        .collect()
}

/// The same from files to files (omr_deskew_with_hough_batch_streams): baseline JPEG or PNG files in, read as imread reads
/// them (an EXIF-tagged JPEG is turned), JPEG files at `quality` out, with nothing but file contents crossing to the GPU
/// and back.  Returns the angle per file.  A file its decoder refuses or cannot decode, or a scan without any segment,
/// fails the call with that scan's code and names it, and no output file is written.  Not in the reference crate.
pub fn deskew_files_with_hough(
    inputs: &[&str],
    outputs: &[&str],
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
        ffi::omr_deskew_with_hough_batch_streams(streams, len, n, 3, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), 0, quality, angles, scan_rc, jpeg, jpeg_len)
    })
}

/// `deskew_files_with_hough` with CCITT Group 4 TIFF files as its outputs (omr_deskew_with_hough_batch_streams_tiff): a
/// pixel is white iff its gray value is above `threshold` (0 .. 254); `rows_per_strip` 0: one strip a page; `dpi` 0: no
/// resolution tags.  Not in the reference crate.
pub fn deskew_files_with_hough_tiff(
    inputs: &[&str],
    outputs: &[&str],
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
        ffi::omr_deskew_with_hough_batch_streams_tiff(streams, len, n, 3, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), threshold, rows_per_strip, dpi, angles, scan_rc, tiff, tiff_len)
    })
}

/// `deskew_files_with_hough` with 8-bit RGB TIFF files as its outputs (omr_deskew_with_hough_batch_streams_tiff8):
/// `compression` 1 (none) or 5 (LZW), `predictor` 1, or 2 with LZW; `rows_per_strip` 0: strips of at most 8192 raw bytes;
/// `dpi` 0: no resolution tags.  Not in the reference crate.
pub fn deskew_files_with_hough_tiff8(
    inputs: &[&str],
    outputs: &[&str],
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
        ffi::omr_deskew_with_hough_batch_streams_tiff8(streams, len, n, 3, min_line_length, max_line_gap, flags, border_mode, border.as_ptr(), clip_strategy.to_abi(), compression, predictor, rows_per_strip, dpi, angles, scan_rc, tiff, tiff_len)
    })
}
