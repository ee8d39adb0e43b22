//! `oics::projection` (reference: packages/lib/src/projection.rs:17-194) -> omr_get_angle_with_projections,
//! its batch form omr_get_angles_with_projections_batch, the batch that also rotates the full-size images,
//! omr_deskew_with_projections_batch, and that flow from files to files, omr_deskew_with_projections_batch_streams.
use crate::bridge::{border_bytes, check, into_mat, view};
use crate::ffi;
use crate::transfer::TransformableMatrix;
use opencv::core::{Mat, Scalar};

/// Scale, gray, threshold, sweep -N..N candidates of `angle_step`, arg-max with the reference's tie policy.
/// `threads` is accepted and ignored: the reference's multi-thread branch rotates by the integer index
/// instead of index * step (projection.rs:94) and no caller uses it.  Panics where the reference panics
/// (`.expect`, projection.rs:26-31,57,61), because the signature has no error channel.
pub fn get_angle_with_projections(
    src: &TransformableMatrix,
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    threads: usize,
) -> f64 {
    let v = view(src.get_mat()).expect("8-bit image");
    let mut angle = 0.0f64;
    let rc = unsafe { ffi::omr_get_angle_with_projections(&v, max_angle, angle_step, resize_scale, threads, &mut angle) };
    if rc != ffi::OMR_OK {
        crate::bridge::check(rc).expect("get_angle_with_projections");
    }
    angle
}

/// `get_angle_with_projections` for a batch: images of any mix of shapes, one angle per image at the image's own
/// position, each the angle the per-call function returns (same f64 bits).  Same-shape images are resized and swept
/// together on the device.  Panics where `get_angle_with_projections` panics; an invalid image fails the whole batch.
pub fn get_angles_with_projections(
    srcs: &[&TransformableMatrix],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
) -> Vec<f64> {
    let views: Vec<ffi::OmrImage> = srcs.iter().map(|s| view(s.get_mat()).expect("8-bit image")).collect();
    let mut angles = vec![0.0f64; srcs.len()];
    let rc = unsafe {
        ffi::omr_get_angles_with_projections_batch(views.as_ptr(), srcs.len() as i32, max_angle, angle_step, resize_scale, angles.as_mut_ptr(), std::ptr::null_mut())
    };
    if rc != ffi::OMR_OK {
        crate::bridge::check(rc).expect("get_angles_with_projections");
    }
    angles
}

/// The reference benchmark's flow (core/src/main.rs:68-95) for a batch -> omr_deskew_with_projections_batch:
/// `get_angle_with_projections(src, max_angle, angle_step, resize_scale, _)` on every image, then
/// `rotate_mat(src, angle, 1.0, flags, BORDER_CONSTANT, border_value, CONTAIN)` of the full-size image.  Images of any mix
/// of shapes; pair i belongs to `srcs[i]`: the per-call angle (same f64 bits) and the rotated image (same bytes).
/// `flags` is INTER_NEAREST (0) or INTER_LINEAR (1); anything else is OMR_ERR_NOTIMPL.
pub fn deskew_with_projections(
    srcs: &[&TransformableMatrix],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    flags: i32,
    border_value: Scalar,
) -> opencv::Result<Vec<(f64, Mat)>> {
    let mut views = Vec::with_capacity(srcs.len());
    for s in srcs {
        views.push(view(s.get_mat())?);
    }
    let border = border_bytes(border_value);
    let mut angles = vec![0.0f64; srcs.len()];
    let mut outs: Vec<ffi::OmrImageOwned> = (0..srcs.len()).map(|_| ffi::OmrImageOwned::empty()).collect();
    check(unsafe {
        ffi::omr_deskew_with_projections_batch(views.as_ptr(), srcs.len() as i32, max_angle, angle_step, resize_scale, flags, border.as_ptr(), angles.as_mut_ptr(), std::ptr::null_mut(), outs.as_mut_ptr())
    })?;
    // every image is taken over before the first error is reported, so none of the library's buffers is lost
    let mats: Vec<opencv::Result<Mat>> = outs.into_iter().map(into_mat).collect();
    mats.into_iter().zip(angles).map(|(m, a)| Ok((a, m?))).collect()
}

/// `std::fs::read` per input, the one batch call `run` (streams in, streams out), then `std::fs::write` per output.  All or
/// nothing: no file is written unless every scan was decoded and deskewed; every stream is released with omr_bytes_free
/// on every path.
pub(crate) fn files_through<F>(inputs: &[&str], outputs: &[&str], run: F) -> opencv::Result<Vec<f64>>
where
    F: FnOnce(*mut *const u8, *const i64, i32, *mut f64, *mut i32, *mut *mut u8, *mut i64) -> i32,
{
    if inputs.len() != outputs.len() || inputs.is_empty() {
        return Err(opencv::Error::new(ffi::OMR_ERR_BADARG, String::from("inputs and outputs must pair up")));
    }
    let n = inputs.len();
    let mut files: Vec<Vec<u8>> = Vec::with_capacity(n);
    for (i, path) in inputs.iter().enumerate() {
        files.push(std::fs::read(path).map_err(|e| opencv::Error::new(ffi::OMR_ERR_BADARG, format!("{} (input {}): {}", path, i, e)))?);
    }
    let mut ptrs: Vec<*const u8> = files.iter().map(|f| f.as_ptr()).collect();
    let lens: Vec<i64> = files.iter().map(|f| f.len() as i64).collect();
    let mut angles = vec![0.0f64; n];
    let mut scan_rc = vec![0i32; n];
    let mut streams: Vec<*mut u8> = vec![std::ptr::null_mut(); n];
    let mut stream_len = vec![0i64; n];
    check(run(ptrs.as_mut_ptr(), lens.as_ptr(), n as i32, angles.as_mut_ptr(), scan_rc.as_mut_ptr(), streams.as_mut_ptr(), stream_len.as_mut_ptr()))?;
    let mut result: opencv::Result<()> = match (0..n).find(|&i| scan_rc[i] != 0) {
        Some(i) => Err(opencv::Error::new(scan_rc[i], format!("the batch deskew failed on {} (scan {}): the JPEG / PNG decoder or the deskew answered {}; no output file was written", inputs[i], i, scan_rc[i]))),
        None => Ok(()),
    };
    for i in 0..n {
        if streams[i].is_null() {
            continue;
        }
        if result.is_ok() {
            let bytes = unsafe { std::slice::from_raw_parts(streams[i], stream_len[i] as usize) };
            if let Err(e) = std::fs::write(outputs[i], bytes) {
                result = Err(opencv::Error::new(ffi::OMR_ERR_BADARG, format!("{} (output {}; outputs before it are written): {}", outputs[i], i, e)));
            }
        }
        unsafe { ffi::omr_bytes_free(streams[i]) };
    }
    result?;
    Ok(angles)
}

/// The reference benchmark's whole loop (core/src/main.rs:68-95: imread, `get_angle_with_projections`, `rotate_mat` of the
/// original with CONTAIN, `im_write(.., JPEG, quality)`) for many files at once, with nothing but file contents crossing
/// to the GPU and back (omr_deskew_with_projections_batch_streams).  Inputs are baseline JPEG or PNG files, told apart by
/// PNG's signature; one batch may hold both.  Returns the angle per file (the per-call function's f64 bits); output i is
/// byte for byte what the per-call chain encodes for input i.  A scan its decoder refuses (progressive JPEG, interlaced
/// PNG, ..: OMR_ERR_NOTIMPL) or cannot decode fails the call with that scan's code and names it, and no output file is
/// written: the caller sends such files through `deskew_with_projections`, whose imread takes them.  Not in the
/// reference crate.
pub fn deskew_files_with_projections(
    inputs: &[&str],
    outputs: &[&str],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    flags: i32,
    border_value: Scalar,
    quality: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, jpeg, jpeg_len| unsafe {
        ffi::omr_deskew_with_projections_batch_streams(streams, len, n, 3, max_angle, angle_step, resize_scale, flags, border.as_ptr(), quality, angles, std::ptr::null_mut(), scan_rc, jpeg, jpeg_len)
    })
}

/// `deskew_files_with_projections` with lossless outputs (omr_deskew_with_projections_batch_streams_png): JPEG or PNG
/// files in, PNG files out.  `compression` is imwrite's IMWRITE_PNG_COMPRESSION (0: stored blocks, 1 .. 9: the one
/// compressed method).  Not in the reference crate.
pub fn deskew_files_with_projections_png(
    inputs: &[&str],
    outputs: &[&str],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    flags: i32,
    border_value: Scalar,
    compression: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, png, png_len| unsafe {
        ffi::omr_deskew_with_projections_batch_streams_png(streams, len, n, 3, max_angle, angle_step, resize_scale, flags, border.as_ptr(), compression, angles, std::ptr::null_mut(), scan_rc, png, png_len)
    })
}

/// `deskew_files_with_projections` with bilevel outputs (omr_deskew_with_projections_batch_streams_tiff): JPEG, PNG or
/// TIFF files in, CCITT Group 4 TIFF files out, a pixel white iff its gray value is above `threshold` (0 .. 254), the
/// strips byte for byte libtiff's.  `rows_per_strip` 0: one strip a page; `dpi` 0: no resolution tags.  Not in the
/// reference crate.
pub fn deskew_files_with_projections_tiff(
    inputs: &[&str],
    outputs: &[&str],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    flags: i32,
    border_value: Scalar,
    threshold: i32,
    rows_per_strip: i32,
    dpi: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, tiff, tiff_len| unsafe {
        ffi::omr_deskew_with_projections_batch_streams_tiff(streams, len, n, 3, max_angle, angle_step, resize_scale, flags, border.as_ptr(), threshold, rows_per_strip, dpi, angles, std::ptr::null_mut(), scan_rc, tiff, tiff_len)
    })
}

/// `deskew_files_with_projections` with 8-bit RGB TIFF files as its outputs
/// (omr_deskew_with_projections_batch_streams_tiff8): the canvases with their levels intact, `compression` 1 (none) or 5
/// (LZW), `predictor` 1, or 2 with LZW.  `rows_per_strip` 0: strips of at most 8192 raw bytes; `dpi` 0: no resolution
/// tags.  Not in the reference crate.
pub fn deskew_files_with_projections_tiff8(
    inputs: &[&str],
    outputs: &[&str],
    max_angle: u16,
    angle_step: f64,
    resize_scale: f64,
    flags: i32,
    border_value: Scalar,
    compression: i32,
    predictor: i32,
    rows_per_strip: i32,
    dpi: i32,
) -> opencv::Result<Vec<f64>> {
    let border = border_bytes(border_value);
    files_through(inputs, outputs, |streams, len, n, angles, scan_rc, tiff, tiff_len| unsafe {
        ffi::omr_deskew_with_projections_batch_streams_tiff8(streams, len, n, 3, max_angle, angle_step, resize_scale, flags, border.as_ptr(), compression, predictor, rows_per_strip, dpi, angles, std::ptr::null_mut(), scan_rc, tiff, tiff_len)
    })
}
