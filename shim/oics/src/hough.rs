//! `oics::hough` (reference: packages/lib/src/hough.rs:17-100) -> omr_get_angle_with_hough / _ex.
use crate::bridge::{check, into_mat, view};
use crate::ffi;
use crate::transfer::TransformableMatrix;
use opencv::core::Vector;
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
