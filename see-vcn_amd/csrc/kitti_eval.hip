// KITTI AP evaluation (detector3d/pcdet/datasets/kitti/kitti_object_eval_python/eval.py, rotate_iou.py) on the device:
//   k_kitti_overlaps      ragged per-frame overlap blocks of one metric, one thread per (detection, ground truth) pair of the SAME frame
//   k_kitti_match_scores  pass 1 of compute_statistics_jit (compute_fp=False): one wave per (frame, combination)
//   k_kitti_thresholds    get_thresholds, one lane per combination, fp64
//   k_kitti_match_stats   pass 2 (compute_fp=True): one wave per (frame, combination, threshold)
//   k_kitti_stats_table   the (combination, 41, 4) table; the similarity column is summed in ascending frame order, no float atomics
// A combination is (class, difficulty, min-overlap row); the ignored_gt / ignored_dt tables depend on (class, difficulty) only (`combo_cd`).
#include <limits.h>

#include "wave.h"

#define KE_PTS 41            // N_SAMPLE_PTS
#define KE_MAX_DT 4096       // detections of one frame: 64 lanes x the 64 bits of a lane's "assigned" word
#define KE_CAP 8             // points of the intersection polygon buffer (rotate_iou.py:235, 16 floats)
#define KE_NO_DETECTION (-10000000.0)

// ------------------------------------------------------------------------------------------------------------------------------------------
// rotate_iou.py:17-260 in fp32, statement for statement (the library is built with -ffp-contract=off and correctly rounded divide / sqrt)
// ------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ke_triangle_area(const float* a, const float* b, const float* c) {
  return ((a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0])) / 2.0f;
}

__device__ __forceinline__ float ke_area(const float* int_pts, int num_of_inter) {
  float area_val = 0.0f;
  for (int i = 0; i < num_of_inter - 2; ++i) area_val += fabsf(ke_triangle_area(int_pts, int_pts + 2 * i + 2, int_pts + 2 * i + 4));
  return area_val;
}

__device__ __forceinline__ void ke_sort_vertex_in_convex_polygon(float* int_pts, int num_of_inter) {
  if (num_of_inter <= 0) return;
  float center[2] = {0.0f, 0.0f};
  for (int i = 0; i < num_of_inter; ++i) {
    center[0] += int_pts[2 * i];
    center[1] += int_pts[2 * i + 1];
  }
  center[0] /= (float)num_of_inter;
  center[1] /= (float)num_of_inter;
  float vs[KE_CAP];
  for (int i = 0; i < num_of_inter; ++i) {
    float v0 = int_pts[2 * i] - center[0];
    float v1 = int_pts[2 * i + 1] - center[1];
    const float d = sqrtf(v0 * v0 + v1 * v1);
    v0 = v0 / d;
    v1 = v1 / d;
    if (v1 < 0) v0 = -2 - v0;
    vs[i] = v0;
  }
  for (int i = 1; i < num_of_inter; ++i) {
    if (vs[i - 1] > vs[i]) {
      const float temp = vs[i], tx = int_pts[2 * i], ty = int_pts[2 * i + 1];
      int j = i;
      while (j > 0 && vs[j - 1] > temp) {
        vs[j] = vs[j - 1];
        int_pts[j * 2] = int_pts[j * 2 - 2];
        int_pts[j * 2 + 1] = int_pts[j * 2 - 1];
        --j;
      }
      vs[j] = temp;
      int_pts[j * 2] = tx;
      int_pts[j * 2 + 1] = ty;
    }
  }
}

__device__ __forceinline__ bool ke_line_segment_intersection(const float* pts1, const float* pts2, int i, int j, float* temp_pts) {
  const float A0 = pts1[2 * i], A1 = pts1[2 * i + 1];
  const float B0 = pts1[2 * ((i + 1) % 4)], B1 = pts1[2 * ((i + 1) % 4) + 1];
  const float C0 = pts2[2 * j], C1 = pts2[2 * j + 1];
  const float D0 = pts2[2 * ((j + 1) % 4)], D1 = pts2[2 * ((j + 1) % 4) + 1];
  const float BA0 = B0 - A0, BA1 = B1 - A1, DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
  const bool acd = DA1 * CA0 > CA1 * DA0;
  const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
  if (acd != bcd) {
    const bool abc = CA1 * BA0 > BA1 * CA0;
    const bool abd = DA1 * BA0 > BA1 * DA0;
    if (abc != abd) {
      const float DC0 = D0 - C0, DC1 = D1 - C1;
      const float ABBA = A0 * B1 - B0 * A1;
      const float CDDC = C0 * D1 - D0 * C1;
      const float DH = BA1 * DC0 - BA0 * DC1;
      const float Dx = ABBA * DC0 - BA0 * CDDC;
      const float Dy = ABBA * DC1 - BA1 * CDDC;
      temp_pts[0] = Dx / DH;
      temp_pts[1] = Dy / DH;
      return true;
    }
  }
  return false;
}

__device__ __forceinline__ bool ke_point_in_quadrilateral(float pt_x, float pt_y, const float* corners) {
  const float ab0 = corners[2] - corners[0], ab1 = corners[3] - corners[1];
  const float ad0 = corners[6] - corners[0], ad1 = corners[7] - corners[1];
  const float ap0 = pt_x - corners[0], ap1 = pt_y - corners[1];
  const float abab = ab0 * ab0 + ab1 * ab1;
  const float abap = ab0 * ap0 + ab1 * ap1;
  const float adad = ad0 * ad0 + ad1 * ad1;
  const float adap = ad0 * ap0 + ad1 * ap1;
  return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

// The reference's buffer holds KE_CAP points and a degenerate pair (identical boxes, a corner on an edge) can present more candidates: it then
// writes past its local array.  Here a candidate that finds the buffer full is dropped.
__device__ __forceinline__ int ke_quadrilateral_intersection(const float* pts1, const float* pts2, float* int_pts) {
  int num_of_inter = 0;
  for (int i = 0; i < 4; ++i) {
    if (ke_point_in_quadrilateral(pts1[2 * i], pts1[2 * i + 1], pts2) && num_of_inter < KE_CAP) {
      int_pts[num_of_inter * 2] = pts1[2 * i];
      int_pts[num_of_inter * 2 + 1] = pts1[2 * i + 1];
      ++num_of_inter;
    }
    if (ke_point_in_quadrilateral(pts2[2 * i], pts2[2 * i + 1], pts1) && num_of_inter < KE_CAP) {
      int_pts[num_of_inter * 2] = pts2[2 * i];
      int_pts[num_of_inter * 2 + 1] = pts2[2 * i + 1];
      ++num_of_inter;
    }
  }
  float temp_pts[2];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      if (ke_line_segment_intersection(pts1, pts2, i, j, temp_pts) && num_of_inter < KE_CAP) {
        int_pts[num_of_inter * 2] = temp_pts[0];
        int_pts[num_of_inter * 2 + 1] = temp_pts[1];
        ++num_of_inter;
      }
  return num_of_inter;
}

// rbbox: centre x, centre y, x_d, y_d, angle
__device__ __forceinline__ void ke_rbbox_to_corners(float* corners, float center_x, float center_y, float x_d, float y_d, float angle) {
  const float a_cos = cosf(angle), a_sin = sinf(angle);
  const float corners_x[4] = {-x_d / 2, -x_d / 2, x_d / 2, x_d / 2};
  const float corners_y[4] = {-y_d / 2, y_d / 2, y_d / 2, -y_d / 2};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    corners[2 * i] = a_cos * corners_x[i] + a_sin * corners_y[i] + center_x;
    corners[2 * i + 1] = -a_sin * corners_x[i] + a_cos * corners_y[i] + center_y;
  }
}

// devRotateIoUEval(rbox1, rbox2, criterion), boxes as five floats each
__device__ __forceinline__ float ke_rotate_iou_eval(const float* rbox1, const float* rbox2, int criterion) {
  const float area1 = rbox1[2] * rbox1[3];
  const float area2 = rbox2[2] * rbox2[3];
  float corners1[8], corners2[8], intersection_corners[2 * KE_CAP];
  ke_rbbox_to_corners(corners1, rbox1[0], rbox1[1], rbox1[2], rbox1[3], rbox1[4]);
  ke_rbbox_to_corners(corners2, rbox2[0], rbox2[1], rbox2[2], rbox2[3], rbox2[4]);
  const int num_intersection = ke_quadrilateral_intersection(corners1, corners2, intersection_corners);
  ke_sort_vertex_in_convex_polygon(intersection_corners, num_intersection);
  const float area_inter = ke_area(intersection_corners, num_intersection);
  if (criterion == -1) return area_inter / (area1 + area2 - area_inter);
  if (criterion == 0) return area_inter / area1;
  if (criterion == 1) return area_inter / area2;
  return area_inter;
}

// image_box_overlap (eval.py:86-113) for one pair
__device__ __forceinline__ float ke_image_overlap(const float* box, const float* qbox, int criterion) {
  const float qbox_area = (qbox[2] - qbox[0]) * (qbox[3] - qbox[1]);
  const float iw = fminf(box[2], qbox[2]) - fmaxf(box[0], qbox[0]);
  if (iw > 0) {
    const float ih = fminf(box[3], qbox[3]) - fmaxf(box[1], qbox[1]);
    if (ih > 0) {
      float ua;
      if (criterion == -1) ua = (box[2] - box[0]) * (box[3] - box[1]) + qbox_area - iw * ih;
      else if (criterion == 0) ua = (box[2] - box[0]) * (box[3] - box[1]);
      else if (criterion == 1) ua = qbox_area;
      else ua = 1.0f;
      return iw * ih / ua;
    }
  }
  return 0.0f;
}

// Segment s owns rows [row_off[s], row_off[s+1]) and columns [col_off[s], col_off[s+1]); its (rows, cols) block starts at out[out_off[s]].
// metric 0: boxes of 4 floats; 1: (x, z, l, w, ry); 2: (x, y, z, l, h, w, ry).  out[n, k] = f(row n, col k) with the reference's argument roles:
// image_box_overlap(boxes = rows, query = cols); devRotateIoUEval(rbox1 = col, rbox2 = row) as rotate_iou_kernel_eval calls it.
__global__ __launch_bounds__(256) void k_kitti_overlaps(const float* __restrict__ row_boxes, const float* __restrict__ col_boxes,
                                                        const int64_t* __restrict__ row_off, const int64_t* __restrict__ col_off,
                                                        const int64_t* __restrict__ out_off, int num_segments, int64_t total_pairs, int metric,
                                                        int criterion, float* __restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total_pairs; p += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = num_segments;                 // the segment s with out_off[s] <= p < out_off[s + 1] (empty segments are stepped over)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (out_off[mid] <= p) lo = mid; else hi = mid;
    }
    const int s = lo;
    const int64_t local = p - out_off[s], ncol = col_off[s + 1] - col_off[s];
    const int64_t n = row_off[s] + local / ncol, k = col_off[s] + local % ncol;
    float v;
    if (metric == 0) {
      v = ke_image_overlap(row_boxes + 4 * n, col_boxes + 4 * k, criterion);
    } else if (metric == 1) {
      float rb[5], qb[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) rb[i] = row_boxes[5 * n + i], qb[i] = col_boxes[5 * k + i];
      v = ke_rotate_iou_eval(qb, rb, criterion);
    } else {
      const float* b = row_boxes + 7 * n;
      const float* q = col_boxes + 7 * k;
      const float rb[5] = {b[0], b[2], b[3], b[5], b[6]}, qb[5] = {q[0], q[2], q[3], q[5], q[6]};
      v = ke_rotate_iou_eval(qb, rb, 2);
      if (v > 0) {                                   // d3_box_overlap_kernel (eval.py:121-147)
        const float iw = fminf(b[1], q[1]) - fmaxf(b[1] - b[4], q[1] - q[4]);
        if (iw > 0) {
          const float area1 = b[3] * b[4] * b[5], area2 = q[3] * q[4] * q[5];
          const float inc = iw * v;
          float ua;
          if (criterion == -1) ua = area1 + area2 - inc;
          else if (criterion == 0) ua = area1;
          else if (criterion == 1) ua = area2;
          else ua = inc;
          v = inc / ua;
        } else {
          v = 0.0f;
        }
      }
    }
    out[p] = v;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// matching
// ------------------------------------------------------------------------------------------------------------------------------------------
struct KeFrame {
  int nd, ng;
  int64_t d0, g0;
  const float* ov;             // (nd, ng) block
  const int8_t* igd;           // ignored_det of this (class, difficulty), this frame
  const int8_t* igg;
  const double* sc;
};

__device__ __forceinline__ KeFrame ke_frame(int f, int cd, const float* overlaps, const int64_t* dt_off, const int64_t* gt_off, const int64_t* ov_off,
                                            const double* dt_scores, const int8_t* ignored_dt, const int8_t* ignored_gt, int64_t total_dt,
                                            int64_t total_gt) {
  KeFrame fr;
  fr.d0 = dt_off[f], fr.g0 = gt_off[f];
  fr.nd = (int)(dt_off[f + 1] - fr.d0), fr.ng = (int)(gt_off[f + 1] - fr.g0);
  fr.ov = overlaps + ov_off[f];
  fr.igd = ignored_dt + (int64_t)cd * total_dt + fr.d0;
  fr.igg = ignored_gt + (int64_t)cd * total_gt + fr.g0;
  fr.sc = dt_scores + fr.d0;
  return fr;
}

// Pass 1 (eval.py:192-242 with compute_fp=False).  Detection j = lane + 64 k lives in lane `lane`, bit k of its `assigned` word.  For a ground truth
// the reference keeps the first detection of the highest score (its `>` is strict): max score over the wave, then the lowest index that has it.
__global__ __launch_bounds__(256) void k_kitti_match_scores(const float* __restrict__ overlaps, const int64_t* __restrict__ dt_off,
                                                            const int64_t* __restrict__ gt_off, const int64_t* __restrict__ ov_off, int num_frames,
                                                            const double* __restrict__ dt_scores, const int8_t* __restrict__ ignored_dt,
                                                            const int8_t* __restrict__ ignored_gt, const int32_t* __restrict__ combo_cd,
                                                            const double* __restrict__ min_overlaps, int num_combos, int64_t total_dt,
                                                            int64_t total_gt, double* __restrict__ tp_scores, int32_t* __restrict__ tp_count) {
  const int lane = threadIdx.x & (SV_WAVE - 1);
  const int64_t w = (int64_t)blockIdx.x * (blockDim.x / SV_WAVE) + threadIdx.x / SV_WAVE;
  if (w >= (int64_t)num_frames * num_combos) return;                   // whole waves leave; the kernel has no barrier
  const int f = (int)(w / num_combos), c = (int)(w % num_combos);
  const KeFrame fr = ke_frame(f, combo_cd[c], overlaps, dt_off, gt_off, ov_off, dt_scores, ignored_dt, ignored_gt, total_dt, total_gt);
  const double mo = min_overlaps[c];
  double* out = tp_scores + (int64_t)c * total_gt + fr.g0;
  unsigned long long assigned = 0;
  int ntp = 0;
  for (int i = 0; i < fr.ng; ++i) {
    const int ig = fr.igg[i];
    if (ig == -1) continue;
    double best = KE_NO_DETECTION;
    int bj = INT_MAX;
    for (int k = 0, j = lane; j < fr.nd; ++k, j += SV_WAVE) {
      if (fr.igd[j] == -1 || ((assigned >> k) & 1ull)) continue;
      if ((double)fr.ov[(int64_t)j * fr.ng + i] > mo) {
        const double s = fr.sc[j];
        if (s > best) best = s, bj = j;
      }
    }
    const double wbest = sv_wave_reduce_max(best);
    const int wj = sv_wave_reduce_min((bj != INT_MAX && best == wbest) ? bj : INT_MAX);
    if (wj == INT_MAX) continue;
    if ((wj & (SV_WAVE - 1)) == lane) assigned |= 1ull << (wj / SV_WAVE);
    if (ig == 1 || fr.igd[wj] == 1) continue;
    if (lane == 0) out[ntp] = wbest;
    ++ntp;
  }
  if (lane == 0 && ntp > 0) atomicAdd(&tp_count[c], ntp);
}

// get_thresholds (eval.py:9-27) on scores already sorted in descending order, one lane per combination.
__global__ void k_kitti_thresholds(const double* __restrict__ sorted_scores, int64_t row_stride, const int32_t* __restrict__ counts,
                                   const int32_t* __restrict__ num_valid_gt, int num_combos, double* __restrict__ thresholds,
                                   int32_t* __restrict__ num_thresholds) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= num_combos) return;
  const double* scores = sorted_scores + (int64_t)c * row_stride;
  const int n = counts[c];
  const double num_gt = (double)num_valid_gt[c];
  double current_recall = 0;
  int nt = 0;
  for (int i = 0; i < n; ++i) {
    const double l_recall = (double)(i + 1) / num_gt;
    double r_recall;
    if (i < n - 1) r_recall = (double)(i + 2) / num_gt;
    else r_recall = l_recall;
    if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
    if (nt < KE_PTS) thresholds[c * KE_PTS + nt] = scores[i];          // a 42nd cannot arise while n <= num_gt; never write past the row
    if (nt < KE_PTS) ++nt;
    current_recall += 1 / (KE_PTS - 1.0);
  }
  num_thresholds[c] = nt;
}

// Pass 2 (compute_fp=True), one wave per (frame, combination, threshold).  With min_overlap >= 0 the inner loop of eval.py:200-225 has a closed form:
// the first eligible unignored detection is always taken (its overlap > min_overlap >= 0 = the initial max_overlap, or an ignored one was taken
// before it), later unignored ones only on a strictly larger overlap, and an ignored one only while nothing is chosen.  So: the eligible
// unignored detection of the largest overlap, lowest index on ties; if there is none, the first eligible ignored one.
__global__ __launch_bounds__(256) void k_kitti_match_stats(const float* __restrict__ overlaps, const int64_t* __restrict__ dt_off,
                                                           const int64_t* __restrict__ gt_off, const int64_t* __restrict__ ov_off, int num_frames,
                                                           const double* __restrict__ dt_scores, const int8_t* __restrict__ ignored_dt,
                                                           const int8_t* __restrict__ ignored_gt, const int32_t* __restrict__ combo_cd,
                                                           const double* __restrict__ min_overlaps, int num_combos, int64_t total_dt,
                                                           int64_t total_gt, const double* __restrict__ thresholds,
                                                           const int32_t* __restrict__ num_thresholds, int metric, int compute_aos,
                                                           const float* __restrict__ dt_bbox, const float* __restrict__ dc_boxes,
                                                           const int64_t* __restrict__ dc_off, const double* __restrict__ gt_alpha,
                                                           const double* __restrict__ dt_alpha, int32_t* __restrict__ counts,
                                                           double* __restrict__ sim_part) {
  const int lane = threadIdx.x & (SV_WAVE - 1);
  const int f = blockIdx.x / num_combos, c = blockIdx.x % num_combos;
  const int t = blockIdx.y * (blockDim.x / SV_WAVE) + threadIdx.x / SV_WAVE;
  if (t >= num_thresholds[c]) return;                                  // whole waves leave; the kernel has no barrier
  const KeFrame fr = ke_frame(f, combo_cd[c], overlaps, dt_off, gt_off, ov_off, dt_scores, ignored_dt, ignored_gt, total_dt, total_gt);
  const double mo = min_overlaps[c], thresh = thresholds[c * KE_PTS + t];
  unsigned long long assigned = 0;
  int tp = 0, fn = 0;
  double similarity = 0.0;
  for (int i = 0; i < fr.ng; ++i) {
    const int ig = fr.igg[i];
    if (ig == -1) continue;
    float bo = -1.0f;
    int bj = INT_MAX, fj = INT_MAX;
    for (int k = 0, j = lane; j < fr.nd; ++k, j += SV_WAVE) {
      const int id = fr.igd[j];
      if (id == -1 || ((assigned >> k) & 1ull) || fr.sc[j] < thresh) continue;
      const float o = fr.ov[(int64_t)j * fr.ng + i];
      if (!((double)o > mo)) continue;
      if (id == 0) {
        if (o > bo) bo = o, bj = j;
      } else if (j < fj) {
        fj = j;
      }
    }
    const float wbo = sv_wave_reduce_max(bo);
    int wj = sv_wave_reduce_min((bj != INT_MAX && bo == wbo) ? bj : INT_MAX);
    bool det_ignored = false;
    if (wj == INT_MAX) {
      wj = sv_wave_reduce_min(fj);
      det_ignored = true;
    }
    if (wj == INT_MAX) {
      if (ig == 0) ++fn;
      continue;
    }
    if ((wj & (SV_WAVE - 1)) == lane) assigned |= 1ull << (wj / SV_WAVE);
    if (ig == 1 || det_ignored) continue;
    ++tp;
    if (compute_aos) similarity += (1.0 + cos(gt_alpha[fr.g0 + i] - dt_alpha[fr.d0 + wj])) / 2.0;
  }
  // false positives; for metric 0 less the "stuff": still-unassigned counted detections that overlap any DontCare box (eval.py:243-262)
  int fp = 0;
  const int64_t c0 = dc_off[f];
  const int ndc = metric == 0 ? (int)(dc_off[f + 1] - c0) : 0;
  for (int k = 0, j = lane; j < fr.nd; ++k, j += SV_WAVE) {
    if (((assigned >> k) & 1ull) || fr.igd[j] != 0 || fr.sc[j] < thresh) continue;
    bool stuff = false;
    for (int q = 0; q < ndc && !stuff; ++q)
      stuff = (double)ke_image_overlap(dt_bbox + 4 * (fr.d0 + j), dc_boxes + 4 * (c0 + q), 0) > mo;
    if (!stuff) ++fp;
  }
  fp = sv_wave_reduce_sum(fp);
  if (lane == 0) {
    int32_t* cnt = counts + ((int64_t)c * KE_PTS + t) * 3;
    if (tp) atomicAdd(cnt, tp);
    if (fp) atomicAdd(cnt + 1, fp);
    if (fn) atomicAdd(cnt + 2, fn);
    if (compute_aos) sim_part[((int64_t)f * num_combos + c) * KE_PTS + t] = similarity;
  }
}

// table[c, t] = (tp, fp, fn, similarity); the similarity of a (combination, threshold) is the sum over the frames in ascending order.
__global__ void k_kitti_stats_table(const int32_t* __restrict__ counts, const double* __restrict__ sim_part,
                                    const int32_t* __restrict__ num_thresholds, int num_frames, int num_combos, int compute_aos,
                                    double* __restrict__ table) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= num_combos * KE_PTS) return;
  const int c = e / KE_PTS, t = e % KE_PTS;
  double s = 0.0;
  const bool live = t < num_thresholds[c];
  if (live && compute_aos)
    for (int f = 0; f < num_frames; ++f) s += sim_part[(int64_t)f * num_combos * KE_PTS + e];
  for (int i = 0; i < 3; ++i) table[4 * (int64_t)e + i] = live ? (double)counts[3 * (int64_t)e + i] : 0.0;
  table[4 * (int64_t)e + 3] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// entries
// ------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int sv_kitti_eval_max_detections(void) { return KE_MAX_DT; }

extern "C" int sv_kitti_overlaps(const float* row_boxes, const float* col_boxes, const int64_t* row_off, const int64_t* col_off,
                                 const int64_t* out_off, int num_segments, int64_t total_pairs, int metric, int criterion, float* out, void* stream) {
  SV_CHECK_ARG(num_segments >= 1 && total_pairs >= 1, "kitti_overlaps: no segment or no pair (the caller skips empty work)");
  SV_CHECK_ARG(metric >= 0 && metric <= 2, "kitti_overlaps: metric %d is none of 0 (image), 1 (bev), 2 (3d)", metric);
  SV_CHECK_ARG(criterion >= -1 && criterion <= (metric == 0 ? 1 : 2), "kitti_overlaps: criterion %d is not defined for metric %d", criterion, metric);
  SV_CHECK_ARG(row_boxes && col_boxes && row_off && col_off && out_off && out, "kitti_overlaps: null pointer");
  SV_CHECK_ARG(sv_on_device(row_boxes) && sv_on_device(col_boxes) && sv_on_device(row_off) && sv_on_device(col_off) && sv_on_device(out_off) &&
               sv_on_device(out), "kitti_overlaps: a pointer is not device memory");
  hipLaunchKernelGGL(k_kitti_overlaps, dim3(sv_grid_1d(total_pairs, 256)), dim3(256), 0, sv_stream(stream), row_boxes, col_boxes, row_off, col_off,
                     out_off, num_segments, total_pairs, metric, criterion, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_kitti_match_scores(const float* overlaps, const int64_t* dt_off, const int64_t* gt_off, const int64_t* ov_off, int num_frames,
                                     const double* dt_scores, const int8_t* ignored_dt, const int8_t* ignored_gt, const int32_t* combo_cd,
                                     const double* min_overlaps, int num_combos, int64_t total_dt, int64_t total_gt, double* tp_scores,
                                     int32_t* tp_count, void* stream) {
  SV_CHECK_ARG(num_frames >= 1 && num_combos >= 1 && total_dt >= 1 && total_gt >= 1, "kitti_match_scores: empty work (the caller skips it)");
  SV_CHECK_ARG((int64_t)num_frames * num_combos <= INT_MAX, "kitti_match_scores: frames x combinations exceeds 2^31 - 1");
  SV_CHECK_ARG(overlaps && dt_off && gt_off && ov_off && dt_scores && ignored_dt && ignored_gt && combo_cd && min_overlaps && tp_scores && tp_count,
               "kitti_match_scores: null pointer");
  SV_CHECK_ARG(sv_on_device(overlaps) && sv_on_device(dt_off) && sv_on_device(gt_off) && sv_on_device(ov_off) && sv_on_device(dt_scores) &&
               sv_on_device(ignored_dt) && sv_on_device(ignored_gt) && sv_on_device(combo_cd) && sv_on_device(min_overlaps) &&
               sv_on_device(tp_scores) && sv_on_device(tp_count), "kitti_match_scores: a pointer is not device memory");
  const int64_t waves = (int64_t)num_frames * num_combos;
  hipLaunchKernelGGL(k_kitti_match_scores, dim3(sv_div_up(waves, 4)), dim3(256), 0, sv_stream(stream), overlaps, dt_off, gt_off, ov_off, num_frames,
                     dt_scores, ignored_dt, ignored_gt, combo_cd, min_overlaps, num_combos, total_dt, total_gt, tp_scores, tp_count);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_kitti_thresholds(const double* sorted_scores, int64_t row_stride, const int32_t* counts, const int32_t* num_valid_gt,
                                   int num_combos, double* thresholds, int32_t* num_thresholds, void* stream) {
  SV_CHECK_ARG(num_combos >= 1 && row_stride >= 1, "kitti_thresholds: empty work (the caller skips it)");
  SV_CHECK_ARG(sorted_scores && counts && num_valid_gt && thresholds && num_thresholds, "kitti_thresholds: null pointer");
  SV_CHECK_ARG(sv_on_device(sorted_scores) && sv_on_device(counts) && sv_on_device(num_valid_gt) && sv_on_device(thresholds) &&
               sv_on_device(num_thresholds), "kitti_thresholds: a pointer is not device memory");
  hipLaunchKernelGGL(k_kitti_thresholds, dim3(sv_div_up(num_combos, 64)), dim3(64), 0, sv_stream(stream), sorted_scores, row_stride, counts,
                     num_valid_gt, num_combos, thresholds, num_thresholds);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_kitti_match_stats(const float* overlaps, const int64_t* dt_off, const int64_t* gt_off, const int64_t* ov_off, int num_frames,
                                    const double* dt_scores, const int8_t* ignored_dt, const int8_t* ignored_gt, const int32_t* combo_cd,
                                    const double* min_overlaps, int num_combos, int64_t total_dt, int64_t total_gt, const double* thresholds,
                                    const int32_t* num_thresholds, int metric, int compute_aos, const float* dt_bbox, const float* dc_boxes,
                                    const int64_t* dc_off, const double* gt_alpha, const double* dt_alpha, int32_t* counts, double* sim_part,
                                    double* table, void* stream) {
  SV_CHECK_ARG(num_frames >= 1 && num_combos >= 1 && total_dt >= 1 && total_gt >= 1, "kitti_match_stats: empty work (the caller skips it)");
  SV_CHECK_ARG((int64_t)num_frames * num_combos <= INT_MAX, "kitti_match_stats: frames x combinations exceeds 2^31 - 1");
  SV_CHECK_ARG(metric >= 0 && metric <= 2, "kitti_match_stats: metric %d is none of 0, 1, 2", metric);
  SV_CHECK_ARG(overlaps && dt_off && gt_off && ov_off && dt_scores && ignored_dt && ignored_gt && combo_cd && min_overlaps && thresholds &&
               num_thresholds && dc_off && counts && table, "kitti_match_stats: null pointer");
  SV_CHECK_ARG(metric != 0 || (dt_bbox && dc_boxes), "kitti_match_stats: metric 0 needs the detections' image boxes and the DontCare boxes");
  SV_CHECK_ARG(!compute_aos || (gt_alpha && dt_alpha && sim_part), "kitti_match_stats: compute_aos needs both alpha arrays and the similarity buffer");
  SV_CHECK_ARG(sv_on_device(overlaps) && sv_on_device(dt_off) && sv_on_device(gt_off) && sv_on_device(ov_off) && sv_on_device(dt_scores) &&
               sv_on_device(ignored_dt) && sv_on_device(ignored_gt) && sv_on_device(combo_cd) && sv_on_device(min_overlaps) &&
               sv_on_device(thresholds) && sv_on_device(num_thresholds) && sv_on_device(dc_off) && sv_on_device(counts) && sv_on_device(table),
               "kitti_match_stats: a pointer is not device memory");
  SV_CHECK_ARG(metric != 0 || (sv_on_device(dt_bbox) && sv_on_device(dc_boxes)), "kitti_match_stats: a box pointer is not device memory");
  SV_CHECK_ARG(!compute_aos || (sv_on_device(gt_alpha) && sv_on_device(dt_alpha) && sv_on_device(sim_part)),
               "kitti_match_stats: an orientation pointer is not device memory");
  hipStream_t st = sv_stream(stream);
  hipLaunchKernelGGL(k_kitti_match_stats, dim3(num_frames * num_combos, sv_div_up(KE_PTS, 4)), dim3(256), 0, st, overlaps, dt_off, gt_off, ov_off,
                     num_frames, dt_scores, ignored_dt, ignored_gt, combo_cd, min_overlaps, num_combos, total_dt, total_gt, thresholds,
                     num_thresholds, metric, compute_aos, dt_bbox, dc_boxes, dc_off, gt_alpha, dt_alpha, counts, sim_part);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kitti_stats_table, dim3(sv_div_up((int64_t)num_combos * KE_PTS, 256)), dim3(256), 0, st, counts, sim_part, num_thresholds,
                     num_frames, num_combos, compute_aos, table);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
