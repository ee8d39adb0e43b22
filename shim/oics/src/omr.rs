//! `oics::omr` (reference: packages/lib/src/omr.rs) over the C ABI.
use crate::bridge::{check, into_mat, view};
use crate::ffi;
use opencv::core::{Mat, Vector};
use opencv::imgcodecs;
use opencv::prelude::*;

/// omr.rs:41-45
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ResultStatus {
    Believed,
    NeedCheck,
    NotAResult,
}

/// omr.rs:46-50
#[derive(Clone, Debug)]
pub struct OmrResult {
    pub angle: f64,
    pub status: ResultStatus,
    pub candidates: Vec<f64>,
}

fn status_of(code: i32) -> ResultStatus {
    match code {
        ffi::OMR_STATUS_BELIEVED => ResultStatus::Believed,
        ffi::OMR_STATUS_NEED_CHECK => ResultStatus::NeedCheck,
        _ => ResultStatus::NotAResult,
    }
}

/// Runs `call` with a growing candidate buffer until every candidate fits.
fn with_candidates<F>(mut call: F) -> opencv::Result<OmrResult>
where
    F: FnMut(*mut f64, *mut i32, *mut f64, i32, *mut i32) -> std::os::raw::c_int,
{
    let mut cap: i32 = 1024;
    loop {
        let mut cand = vec![0.0f64; cap as usize];
        let (mut angle, mut status, mut len) = (0.0f64, 0i32, 0i32);
        check(call(&mut angle, &mut status, cand.as_mut_ptr(), cap, &mut len))?;
        if len <= cap {
            cand.truncate(len as usize);
            return Ok(OmrResult { angle, status: status_of(status), candidates: cand });
        }
        cap = len;
    }
}

/// omr.rs:8-39 -> (horizontal projection [rows], vertical projection [cols]).
pub fn get_mat_projection_data(mat: &Mat) -> opencv::Result<(Vec<f64>, Vec<f64>)> {
    let v = view(mat)?;
    let mut h = vec![0.0f64; v.rows as usize];
    let mut w = vec![0.0f64; v.cols as usize];
    check(unsafe { ffi::omr_get_mat_projection_data(&v, h.as_mut_ptr(), w.as_mut_ptr()) })?;
    Ok((h, w))
}

/// omr.rs:52-229.
pub fn get_result_from_projection(
    src: &Mat,
    projection_max_angle: u16,
    projection_angle_step: f64,
    projection_max_width: i32,
    projection_max_height: i32,
) -> opencv::Result<OmrResult> {
    let v = view(src)?;
    with_candidates(|a, s, c, cap, n| unsafe {
        ffi::omr_get_result_from_projection(&v, projection_max_angle, projection_angle_step, projection_max_width, projection_max_height, a, s, c, cap, n)
    })
}

/// omr.rs:231-302.
pub fn get_result_from_edges_detection(
    src: &Mat,
    edges_min_line_length: f64,
    edges_max_line_gap: f64,
) -> opencv::Result<OmrResult> {
    let v = view(src)?;
    with_candidates(|a, s, c, cap, n| unsafe {
        ffi::omr_get_result_from_edges_detection(&v, edges_min_line_length, edges_max_line_gap, a, s, c, cap, n)
    })
}

/// omr.rs:304-337.
pub fn get_result_from_fourier_transform(
    src: &Mat,
    canny_threshold_weak: f64,
    canny_threshold_strong: f64,
    fourier_min_line_length: f64,
    fourier_max_line_gap: f64,
) -> opencv::Result<OmrResult> {
    let v = view(src)?;
    with_candidates(|a, s, c, cap, n| unsafe {
        ffi::omr_get_result_from_fourier_transform(&v, canny_threshold_weak, canny_threshold_strong, fourier_min_line_length, fourier_max_line_gap, a, s, c, cap, n)
    })
}

/// omr.rs:339-448: imread(COLOR) -> projection, Hough fallback and the decision on the GPU -> CONTAIN warp
/// on the GPU -> imwrite(JPEG, quality 100).  Returns (rotation angle, need_check).
pub fn correct_default(
    input_file: &str,
    output_file: &str,
    projection_max_angle: u16,
    projection_angle_step: f64,
    projection_max_width: i32,
    projection_max_height: i32,
    hough_min_line_length: f64,
    hough_max_line_gap: f64,
) -> opencv::Result<(f64, bool)> {
    let src = imgcodecs::imread(input_file, imgcodecs::IMREAD_COLOR)?;
    let (mut angle, mut need_check) = (0.0f64, 0i32);
    let mut rotated = ffi::OmrImageOwned::empty();
    check(unsafe {
        ffi::omr_correct_default(&view(&src)?, projection_max_angle, projection_angle_step, projection_max_width,
                                 projection_max_height, hough_min_line_length, hough_max_line_gap, &mut angle,
                                 &mut need_check, &mut rotated)
    })?;
    let out = into_mat(rotated)?;
    let params: Vector<i32> = Vector::from_slice(&[imgcodecs::IMWRITE_JPEG_QUALITY, 100]);
    imgcodecs::imwrite(output_file, &out, &params)?;
    Ok((angle, need_check != 0))
}

/// `correct_default` for many files at once (omr_correct_default_batch_jpeg): imread(COLOR) per input on host threads, one
/// batch call that corrects the sheets and encodes every rotated canvas as JPEG (quality 100) on the GPU, then
/// `std::fs::write` per output.  Returns (rotation angle, need_check) per file.  A sheet the per-call function fails on
/// fails the call with that sheet's code, names it, and no output file is written; an output that cannot be written
/// fails the call with its index, the outputs before it being on disk.  Not in the reference crate.
pub fn correct_defaults(
    inputs: &[&str],
    outputs: &[&str],
    projection_max_angle: u16,
    projection_angle_step: f64,
    projection_max_width: i32,
    projection_max_height: i32,
    hough_min_line_length: f64,
    hough_max_line_gap: f64,
) -> opencv::Result<Vec<(f64, bool)>> {
    if inputs.len() != outputs.len() || inputs.is_empty() {
        return Err(opencv::Error::new(ffi::OMR_ERR_BADARG, String::from("inputs and outputs must pair up")));
    }
    let n = inputs.len();
    let threads = n.min(16);
    let mut mats: Vec<opencv::Result<Mat>> = Vec::with_capacity(n);
    std::thread::scope(|sc| {
        let handles: Vec<_> = (0..threads)
            .map(|t| {
                sc.spawn(move || {
                    (t..n).step_by(threads).map(|i| (i, imgcodecs::imread(inputs[i], imgcodecs::IMREAD_COLOR))).collect::<Vec<_>>()
                })
            })
            .collect();
        let mut got: Vec<(usize, opencv::Result<Mat>)> = handles.into_iter().flat_map(|h| h.join().unwrap()).collect();
        got.sort_by_key(|e| e.0);
        mats.extend(got.into_iter().map(|e| e.1));
    });
    let mats: Vec<Mat> = mats.into_iter().collect::<opencv::Result<Vec<_>>>()?;
    let views: Vec<ffi::OmrImage> = mats.iter().map(view).collect::<opencv::Result<Vec<_>>>()?;
    let mut angle = vec![0.0f64; n];
    let (mut need_check, mut scan_rc) = (vec![0i32; n], vec![0i32; n]);
    let mut jpeg: Vec<*mut u8> = vec![std::ptr::null_mut(); n];
    let mut jpeg_len = vec![0i64; n];
    check(unsafe {
        ffi::omr_correct_default_batch_jpeg(views.as_ptr(), n as i32, projection_max_angle, projection_angle_step,
                                            projection_max_width, projection_max_height, hough_min_line_length,
                                            hough_max_line_gap, 100, angle.as_mut_ptr(), need_check.as_mut_ptr(),
                                            scan_rc.as_mut_ptr(), jpeg.as_mut_ptr(), jpeg_len.as_mut_ptr())
    })?;
    // all or nothing: no file is written unless every sheet was corrected
    let failed = (0..n).find(|&i| scan_rc[i] != 0);
    let mut result: opencv::Result<()> = match failed {
        Some(i) => Err(opencv::Error::new(scan_rc[i], format!("correct_default failed on {} (sheet {}); no output file was written", inputs[i], i))),
        None => Ok(()),
    };
    for i in 0..n {
        if jpeg[i].is_null() {
            continue;
        }
        if result.is_ok() {
            let bytes = unsafe { std::slice::from_raw_parts(jpeg[i], jpeg_len[i] as usize) };
            if let Err(e) = std::fs::write(outputs[i], bytes) {
                result = Err(opencv::Error::new(ffi::OMR_ERR_BADARG, format!("{} (output {}; outputs before it are written): {}", outputs[i], i, e)));
            }
        }
        unsafe { ffi::omr_bytes_free(jpeg[i]) };
    }
    result?;
    Ok((0..n).map(|i| (angle[i], need_check[i] != 0)).collect())
}

/// `correct_default` for many files at once with nothing but file contents crossing to the GPU and back
/// (omr_correct_default_batch_streams): `std::fs::read` per input, one batch call that decodes the streams (baseline JPEG
/// or PNG, told apart by PNG's signature; one batch may hold both), corrects the sheets and encodes every rotated canvas
/// as JPEG (quality 100) on the GPU, then `std::fs::write` per output.  Returns (rotation angle, need_check) per file.  A
/// sheet its decoder refuses (progressive or CMYK JPEG, interlaced or 16-bit PNG, an EXIF orientation, ..:
/// OMR_ERR_NOTIMPL) or cannot decode fails the call with that sheet's code and names it, and no output file is written:
/// the caller sends such files through `correct_defaults`, whose imread takes them.  Not in the reference crate.
pub fn correct_default_files(
    inputs: &[&str],
    outputs: &[&str],
    projection_max_angle: u16,
    projection_angle_step: f64,
    projection_max_width: i32,
    projection_max_height: i32,
    hough_min_line_length: f64,
    hough_max_line_gap: f64,
) -> opencv::Result<Vec<(f64, bool)>> {
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
    let mut angle = vec![0.0f64; n];
    let (mut need_check, mut scan_rc) = (vec![0i32; n], vec![0i32; n]);
    let mut jpeg: Vec<*mut u8> = vec![std::ptr::null_mut(); n];
    let mut jpeg_len = vec![0i64; n];
    check(unsafe {
        ffi::omr_correct_default_batch_streams(ptrs.as_mut_ptr(), lens.as_ptr(), n as i32, projection_max_angle,
                                               projection_angle_step, projection_max_width, projection_max_height,
                                               hough_min_line_length, hough_max_line_gap, 100, angle.as_mut_ptr(),
                                               need_check.as_mut_ptr(), scan_rc.as_mut_ptr(), jpeg.as_mut_ptr(),
                                               jpeg_len.as_mut_ptr())
    })?;
    // all or nothing: no file is written unless every sheet was decoded and corrected
    let failed = (0..n).find(|&i| scan_rc[i] != 0);
    let mut result: opencv::Result<()> = match failed {
        Some(i) => Err(opencv::Error::new(scan_rc[i], format!("correct_default failed on {} (sheet {}): the JPEG / PNG decoder or the correction answered {}; no output file was written", inputs[i], i, scan_rc[i]))),
        None => Ok(()),
    };
    for i in 0..n {
        if jpeg[i].is_null() {
            continue;
        }
        if result.is_ok() {
            let bytes = unsafe { std::slice::from_raw_parts(jpeg[i], jpeg_len[i] as usize) };
            if let Err(e) = std::fs::write(outputs[i], bytes) {
                result = Err(opencv::Error::new(ffi::OMR_ERR_BADARG, format!("{} (output {}; outputs before it are written): {}", outputs[i], i, e)));
            }
        }
        unsafe { ffi::omr_bytes_free(jpeg[i]) };
    }
    result?;
    Ok((0..n).map(|i| (angle[i], need_check[i] != 0)).collect())
}

/// The tail of the flow functions that write PNG files: all or nothing -- no file is written unless every sheet was
/// corrected (`what` names the stages that may have answered a code) --, then `std::fs::write` per output; every stream is
/// released with omr_bytes_free on every path.
fn write_streams(inputs: &[&str], outputs: &[&str], scan_rc: &[i32], streams: &[*mut u8], lens: &[i64], what: &str) -> opencv::Result<()> {
    let n = inputs.len();
    let mut result: opencv::Result<()> = match (0..n).find(|&i| scan_rc[i] != 0) {
        Some(i) => Err(opencv::Error::new(scan_rc[i], format!("correct_default failed on {} (sheet {}): {} answered {}; no output file was written", inputs[i], i, what, scan_rc[i]))),
        None => Ok(()),
    };
    for i in 0..n {
        if streams[i].is_null() {
            continue;
        }
        if result.is_ok() {
            let bytes = unsafe { std::slice::from_raw_parts(streams[i], lens[i] as usize) };
            if let Err(e) = std::fs::write(outputs[i], bytes) {
                result = Err(opencv::Error::new(ffi::OMR_ERR_BADARG, format!("{} (output {}; outputs before it are written): {}", outputs[i], i, e)));
            }
        }
        unsafe { ffi::omr_bytes_free(streams[i]) };
    }
    result
}

/// `correct_defaults` with lossless outputs (omr_correct_default_batch_png): imread(COLOR) per input on host threads, one
/// batch call that corrects the sheets and encodes every rotated canvas as PNG (`compression` is imwrite's
/// IMWRITE_PNG_COMPRESSION: 0 stores, 1 .. 9 all compress alike) on the GPU, then `std::fs::write` per output.  Returns
/// (rotation angle, need_check) per file; errors as `correct_defaults`.  Not in the reference crate.
pub fn correct_defaults_png(
    inputs: &[&str],
    outputs: &[&str],
    projection_max_angle: u16,
    projection_angle_step: f64,
    projection_max_width: i32,
    projection_max_height: i32,
    hough_min_line_length: f64,
    hough_max_line_gap: f64,
    compression: i32,
) -> opencv::Result<Vec<(f64, bool)>> {
    if inputs.len() != outputs.len() || inputs.is_empty() {
        return Err(opencv::Error::new(ffi::OMR_ERR_BADARG, String::from("inputs and outputs must pair up")));
    }
    let n = inputs.len();
    let threads = n.min(16);
    let mut mats: Vec<opencv::Result<Mat>> = Vec::with_capacity(n);
    std::thread::scope(|sc| {
        let handles: Vec<_> = (0..threads)
            .map(|t| {
                sc.spawn(move || {
                    (t..n).step_by(threads).map(|i| (i, imgcodecs::imread(inputs[i], imgcodecs::IMREAD_COLOR))).collect::<Vec<_>>()
                })
            })
            .collect();
        let mut got: Vec<(usize, opencv::Result<Mat>)> = handles.into_iter().flat_map(|h| h.join().unwrap()).collect();
        got.sort_by_key(|e| e.0);
        mats.extend(got.into_iter().map(|e| e.1));
    });
    let mats: Vec<Mat> = mats.into_iter().collect::<opencv::Result<Vec<_>>>()?;
    let views: Vec<ffi::OmrImage> = mats.iter().map(view).collect::<opencv::Result<Vec<_>>>()?;
    let mut angle = vec![0.0f64; n];
    let (mut need_check, mut scan_rc) = (vec![0i32; n], vec![0i32; n]);
    let mut png: Vec<*mut u8> = vec![std::ptr::null_mut(); n];
    let mut png_len = vec![0i64; n];
    check(unsafe {
        ffi::omr_correct_default_batch_png(views.as_ptr(), n as i32, projection_max_angle, projection_angle_step,
                                           projection_max_width, projection_max_height, hough_min_line_length,
                                           hough_max_line_gap, compression, angle.as_mut_ptr(), need_check.as_mut_ptr(),
                                           scan_rc.as_mut_ptr(), png.as_mut_ptr(), png_len.as_mut_ptr())
    })?;
    write_streams(inputs, outputs, &scan_rc, &png, &png_len, "the correction")?;
    Ok((0..n).map(|i| (angle[i], need_check[i] != 0)).collect())
}

/// `correct_default_files` with lossless outputs (omr_correct_default_batch_streams_png): JPEG or PNG files in, PNG files
/// out, with nothing but file contents crossing to the GPU and back.  `compression` as for `correct_defaults_png`; errors
/// as `correct_default_files`.  Not in the reference crate.
pub fn correct_default_files_png(
    inputs: &[&str],
    outputs: &[&str],
    projection_max_angle: u16,
    projection_angle_step: f64,
    projection_max_width: i32,
    projection_max_height: i32,
    hough_min_line_length: f64,
    hough_max_line_gap: f64,
    compression: i32,
) -> opencv::Result<Vec<(f64, bool)>> {
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
    let mut angle = vec![0.0f64; n];
    let (mut need_check, mut scan_rc) = (vec![0i32; n], vec![0i32; n]);
    let mut png: Vec<*mut u8> = vec![std::ptr::null_mut(); n];
    let mut png_len = vec![0i64; n];
    check(unsafe {
        ffi::omr_correct_default_batch_streams_png(ptrs.as_mut_ptr(), lens.as_ptr(), n as i32, projection_max_angle,
                                                   projection_angle_step, projection_max_width, projection_max_height,
                                                   hough_min_line_length, hough_max_line_gap, compression, angle.as_mut_ptr(),
                                                   need_check.as_mut_ptr(), scan_rc.as_mut_ptr(), png.as_mut_ptr(),
                                                   png_len.as_mut_ptr())
    })?;
    write_streams(inputs, outputs, &scan_rc, &png, &png_len, "the JPEG / PNG decoder or the correction")?;
    Ok((0..n).map(|i| (angle[i], need_check[i] != 0)).collect())
}
