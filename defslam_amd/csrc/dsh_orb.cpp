// Host side of the ORB front end (include/defslam_hip.h: dsh_orb_create, dsh_orb_destroy, dsh_orb_level_sizes, dsh_orb_detect,
// dsh_orb_describe, dsh_orb_get_plane): the scale table, the level sizes, the resize taps and the cells of every level are computed once
// at create; a detect is one upload of the image, the launches of orb_kernels.hip and one download of counts and candidates; a describe
// is one block up and one down.  The extractor is a device-resident object with the life cycle of the stores (dsh_store).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "orb_problem.h"

struct dsh_orb : dsh_store {
  int32_t width = 0, height = 0, levels = 0, capacity = 0;
  float sf[ORB_MAX_LEVELS] = {}, inv[ORB_MAX_LEVELS] = {};
  int32_t w[ORB_MAX_LEVELS] = {}, h[ORB_MAX_LEVELS] = {};
  char* d_all = nullptr;       // the one device allocation; null on a host-only context
  OrbLevels L = {};
  OrbDetect D = {};            // counts and cand are set per call
  const int32_t* d_pattern = nullptr;
  bool detected = false;
};

namespace {

int cv_round(float v) { return (int)std::rint(v); }

// the taps of one axis: dst entries of 3 (first tap's index, c0, c1)
void resize_taps(int src, int dst, int32_t* tab) {
  const double sc = (double)src / dst;
  for (int d = 0; d < dst; d++) {
    const double t = (d + 0.5) * sc;
    float f = (float)(t - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    tab[3 * d] = s;
    tab[3 * d + 1] = cv_round((1.f - f) * 2048.f);
    tab[3 * d + 2] = cv_round(f * 2048.f);
  }
}

// the cells of a level in the reference's order (ORBextractor.cc:773-806)
void level_cells(int level, int w, int h, std::vector<OrbCell>& cells) {
  const int minB = ORB_FRAME - 3, maxBX = w - ORB_FRAME + 3, maxBY = h - ORB_FRAME + 3;
  const float width = (float)(maxBX - minB), height = (float)(maxBY - minB);
  const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
  const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
  for (int i = 0; i < nRows; i++) {
    const int iniY = minB + i * hCell;
    if (iniY >= maxBY - 3) continue;
    const int maxY = std::min(iniY + hCell + 6, maxBY);
    for (int j = 0; j < nCols; j++) {
      const int iniX = minB + j * wCell;
      if (iniX >= maxBX - 6) continue;
      const int maxX = std::min(iniX + wCell + 6, maxBX);
      cells.push_back({(int16_t)level, 0, (int16_t)iniX, (int16_t)iniY, (int16_t)maxX, (int16_t)maxY});
    }
  }
}

}  // namespace

extern "C" {

int dsh_orb_create(const dsh_orb_config* cfg, dsh_orb** out) {
  if (!cfg) return DSH_ERR_ARG;
  dsh_ctx_base* c = dsh_base(cfg->ctx);
  if (!c) return DSH_ERR_ARG;
  auto bad = [&](const std::string& m) { return dsh_fail(c, DSH_ERR_ARG, "dsh_orb_create: " + m); };
  if (!out) return bad("out is NULL");
  *out = nullptr;
  if (!cfg->pattern) return bad("pattern is NULL");
  if (cfg->levels < 1 || cfg->levels > ORB_MAX_LEVELS) return bad("levels outside 1 .. 32");
  if (!(cfg->scale_factor > 1.0f) || !std::isfinite(cfg->scale_factor)) return bad("scale_factor must be greater than 1");
  if (cfg->min_th_fast < 1 || cfg->min_th_fast > cfg->ini_th_fast || cfg->ini_th_fast > 255) return bad("thresholds outside 1 <= min_th_fast <= ini_th_fast <= 255");
  if (cfg->capacity < 1 || cfg->capacity > (1 << 20)) return bad("capacity outside 1 .. 2^20");
  if (cfg->width < 1 || cfg->height < 1 || cfg->width > 16384 || cfg->height > 16384) return bad("width or height outside 1 .. 16384");
  for (int i = 0; i < ORB_PATTERN_POINTS; i++) {
    const long long x = cfg->pattern[2 * i], y = cfg->pattern[2 * i + 1];
    if (x * x + y * y > ORB_PATTERN_R2) return bad("pattern point " + std::to_string(i) + " has x^2 + y^2 > 342");
  }
  dsh_orb* o = new dsh_orb();
  o->width = cfg->width; o->height = cfg->height; o->levels = cfg->levels; o->capacity = cfg->capacity;
  for (int l = 0; l < o->levels; l++) {   // ORBextractor.cc:415-431, :1124-1125
    o->sf[l] = l == 0 ? 1.0f : o->sf[l - 1] * cfg->scale_factor;
    o->inv[l] = 1.0f / o->sf[l];
    o->w[l] = cv_round((float)o->width * o->inv[l]);
    o->h[l] = cv_round((float)o->height * o->inv[l]);
    if (o->w[l] < ORB_MIN_LEVEL || o->h[l] < ORB_MIN_LEVEL) {
      const std::string m = "level " + std::to_string(l) + " is " + std::to_string(o->w[l]) + " x " + std::to_string(o->h[l]) + ": smaller than 62 pixels, it has no cell";
      delete o;
      return bad(m);
    }
  }
  if (!c->host_only) {
    // a host-only context gets an extractor without arrays: its entry points check arguments and refuse (dsh_enter)
    if (const int rc = dsh_enter(c, "dsh_orb_create")) { delete o; return rc; }
    std::vector<OrbCell> cells;
    std::vector<int32_t> tabs;
    std::vector<size_t> o_plane(o->levels), o_blur(o->levels), o_kept(o->levels), o_xtab(o->levels), o_ytab(o->levels);
    Arena a;
    OrbLevels& L = o->L;
    L.levels = o->levels;
    for (int l = 0; l < o->levels; l++) {
      const int w = o->w[l], h = o->h[l];
      o->D.level_cell0[l] = (int32_t)cells.size();
      level_cells(l, w, h, cells);
      o_plane[l] = a.take((size_t)(w + 2 * ORB_FRAME) * (h + 2 * ORB_FRAME));
      o_blur[l] = a.take((size_t)(w + 2 * ORB_BLUR_MARGIN) * (h + 2 * ORB_BLUR_MARGIN));
      o_kept[l] = a.take((size_t)w * h);
      o_xtab[l] = tabs.size();
      o_ytab[l] = tabs.size() + 3 * (size_t)w;
      tabs.resize(tabs.size() + 3 * (size_t)(w + h));
      if (l > 0) {
        resize_taps(o->w[l - 1], w, &tabs[o_xtab[l]]);
        resize_taps(o->h[l - 1], h, &tabs[o_ytab[l]]);
      }
      L.l[l].w = w; L.l[l].h = h;
      L.l[l].blur_tile0 = L.blur_tiles;
      L.l[l].blur_tiles_x = (w + 2 * ORB_BLUR_MARGIN + ORB_BLUR_TX - 1) / ORB_BLUR_TX;
      L.blur_tiles += L.l[l].blur_tiles_x * ((h + 2 * ORB_BLUR_MARGIN + ORB_BLUR_TY - 1) / ORB_BLUR_TY);
    }
    o->D.level_cell0[o->levels] = (int32_t)cells.size();
    for (int l = o->levels + 1; l <= ORB_MAX_LEVELS; l++) o->D.level_cell0[l] = (int32_t)cells.size();
    for (const OrbCell& k : cells)
      if (k.x1 - k.x0 > ORB_CELL_MAX || k.y1 - k.y0 > ORB_CELL_MAX || k.x1 - k.x0 < 1 || k.y1 - k.y0 < 1) {
        delete o;
        return bad("a cell wider than 65 pixels");   // the cell arithmetic excludes it
      }
    const size_t n_cells = cells.size();
    const size_t o_tabs = a.take(4 * tabs.size()), o_cells = a.take(sizeof(OrbCell) * n_cells), o_pat = a.take(8 * ORB_PATTERN_POINTS),
                 o_count = a.take(4 * n_cells), o_off = a.take(4 * n_cells);
    if (hipMalloc((void**)&o->d_all, a.size) != hipSuccess) {
      delete o;
      return dsh_fail(c, DSH_ERR_HIP, "dsh_orb_create: out of device memory");
    }
    char* d = o->d_all;
    if (hipMemcpy(d + o_tabs, tabs.data(), 4 * tabs.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + o_cells, cells.data(), sizeof(OrbCell) * n_cells, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + o_pat, cfg->pattern, 8 * ORB_PATTERN_POINTS, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(o->d_all);
      delete o;
      return dsh_fail(c, DSH_ERR_HIP, "dsh_orb_create: hipMemcpy failed");
    }
    const int32_t* d_tabs = reinterpret_cast<const int32_t*>(d + o_tabs);
    for (int l = 0; l < o->levels; l++) {
      L.l[l].plane = reinterpret_cast<uint8_t*>(d + o_plane[l]);
      L.l[l].blur = reinterpret_cast<uint8_t*>(d + o_blur[l]);
      L.l[l].kept = reinterpret_cast<uint8_t*>(d + o_kept[l]);
      L.l[l].xtab = l > 0 ? d_tabs + o_xtab[l] : nullptr;
      L.l[l].ytab = l > 0 ? d_tabs + o_ytab[l] : nullptr;
    }
    o->D.cells = reinterpret_cast<const OrbCell*>(d + o_cells);
    o->D.n_cells = (int32_t)n_cells;
    o->D.ini_th = cfg->ini_th_fast; o->D.min_th = cfg->min_th_fast;
    o->D.capacity = o->capacity;
    o->D.cell_count = reinterpret_cast<int32_t*>(d + o_count);
    o->D.cell_offset = reinterpret_cast<int32_t*>(d + o_off);
    o->d_pattern = reinterpret_cast<const int32_t*>(d + o_pat);
  }
  dsh_attach_store(c, o);
  *out = o;
  return DSH_OK;
}

int dsh_orb_destroy(dsh_orb* orb) {
  if (!orb) return DSH_ERR_ARG;
  if (orb->d_all) dsh_store_unregister(orb);
  else if (orb->ctx) orb->ctx->stores.erase(std::remove(orb->ctx->stores.begin(), orb->ctx->stores.end(), (dsh_store*)orb), orb->ctx->stores.end());
  if (orb->d_all) (void)hipFree(orb->d_all);
  delete orb;
  return DSH_OK;
}

int dsh_orb_level_sizes(const dsh_orb* db, int32_t* wh, float* scale) {
  DSH_STORE_ENTER("dsh_orb_level_sizes");
  if (!wh || !scale) return bad("wh or scale is NULL");
  for (int l = 0; l < db->levels; l++) {
    wh[2 * l] = db->w[l];
    wh[2 * l + 1] = db->h[l];
    scale[l] = db->sf[l];
  }
  return DSH_OK;
}

int dsh_orb_detect(dsh_orb* db, const uint8_t* image, int64_t row_stride, int32_t* counts, int32_t* cand) {
  DSH_STORE_ENTER("dsh_orb_detect");
  if (!image || !counts || !cand) return bad("image, counts or cand is NULL");
  if (row_stride < db->width) return bad("row_stride is smaller than the width");
  DSH_STORE_GATE();
  const size_t W = (size_t)db->width, H = (size_t)db->height, nl = (size_t)db->levels, cap = (size_t)db->capacity;
  UpBlock up;
  const bool packed = (size_t)row_stride == W;
  const size_t o_img = packed ? up.copy_of(image, W * H) : up.take(W * H);
  DownBlock down;
  const size_t d_counts = down.take(4 * nl), d_cand = down.take(12 * nl * cap);
  if (const int rc = up.stage(c)) return rc;
  if (!packed)   // the rows without their padding
    for (size_t y = 0; y < H; y++) std::memcpy(up.host<uint8_t>(o_img) + y * W, image + y * (size_t)row_stride, W);
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  hipStream_t st = c->stream;
  const OrbLevels& L = db->L;
  HIPCHK(c, orb_frame_image_launch(L.l[0], up.dev<const uint8_t>(o_img), (int64_t)W, st));
  for (int l = 1; l < db->levels; l++) HIPCHK(c, orb_resize_launch(L.l[l - 1], L.l[l], st));
  HIPCHK(c, orb_blur_launch(L, st));
  OrbDetect D = db->D;
  D.counts = down.dev<int32_t>(d_counts);
  D.cand = down.dev<int32_t>(d_cand);
  HIPCHK(c, orb_fast_launch(L, D, st));
  HIPCHK(c, orb_scan_launch(L, D, st));
  HIPCHK(c, orb_scatter_launch(L, D, st));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st));
  db->detected = true;
  // the candidates' lengths came down with them: the caller gets exactly that many of each level
  const int32_t* hc = down.host<int32_t>(d_counts);
  std::memcpy(counts, hc, 4 * nl);
  int over = -1;
  for (size_t l = 0; l < nl; l++) {
    const size_t n = std::min((size_t)hc[l], cap);
    if (n) std::memcpy(cand + 3 * l * cap, down.host<int32_t>(d_cand) + 3 * l * cap, 12 * n);
    if ((size_t)hc[l] > cap && over < 0) over = (int)l;
  }
  if (over >= 0)
    return bad("level " + std::to_string(over) + " has " + std::to_string(hc[over]) + " candidates, more than the capacity " + std::to_string(db->capacity));
  return DSH_OK;
}

int dsh_orb_describe(dsh_orb* db, int32_t n, const int32_t* level, const float* xy, float* angle, uint8_t* desc) {
  DSH_STORE_ENTER("dsh_orb_describe");
  if (const char* ne = dsh_keypoint_count_error(n)) return bad(ne);
  if (n > 0 && (!level || !xy || !angle || !desc)) return bad("level, xy, angle or desc is NULL");
  for (int i = 0; i < n; i++) {
    const int l = level[i];
    if (l < 0 || l >= db->levels) return bad("key point " + std::to_string(i) + " has a level outside the pyramid");
    const float x = std::rint(xy[2 * (size_t)i]), y = std::rint(xy[2 * (size_t)i + 1]);
    if (!(x >= (float)ORB_EDGE && x <= (float)(db->w[l] - 1 - ORB_EDGE) && y >= (float)ORB_EDGE && y <= (float)(db->h[l] - 1 - ORB_EDGE)))
      return bad("key point " + std::to_string(i) + " lies less than 16 pixels from an edge of its level");
  }
  DSH_STORE_GATE();
  if (!db->detected) return refuse(DSH_ERR_STATE, "no image yet: dsh_orb_detect comes first");
  if (n == 0) return DSH_OK;
  const size_t m = (size_t)n;
  UpBlock up;
  const size_t o_level = up.copy_of(level, 4 * m), o_xy = up.copy_of(xy, 8 * m);
  DownBlock down;
  const size_t d_angle = down.copy_to(angle, 4 * m), d_desc = down.copy_to(desc, 32 * m);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  OrbDescribe D;
  D.n = n;
  D.level = up.dev<const int32_t>(o_level);
  D.xy = up.dev<const float>(o_xy);
  D.pattern = db->d_pattern;
  D.angle = down.dev<float>(d_angle);
  D.desc = down.dev<uint32_t>(d_desc);
  HIPCHK(c, orb_describe_launch(db->L, D, c->stream));
  return down.receive(c);
}

int dsh_orb_get_plane(dsh_orb* db, int32_t level, int32_t blurred, uint8_t* out) {
  DSH_STORE_ENTER("dsh_orb_get_plane");
  if (level < 0 || level >= db->levels) return bad("level outside the pyramid");
  if (!out) return bad("out is NULL");
  DSH_STORE_GATE();
  if (!db->detected) return refuse(DSH_ERR_STATE, "no image yet: dsh_orb_detect comes first");
  const int margin = blurred ? ORB_BLUR_MARGIN : ORB_FRAME;
  const size_t bytes = (size_t)(db->w[level] + 2 * margin) * (db->h[level] + 2 * margin);
  DownBlock down;   // placed over the plane itself: the unpadded slice ends with the allocation's slice
  down.copy_to(down.take_exact(bytes), out, bytes);
  if (const int rc = down.at(c, blurred ? db->L.l[level].blur : db->L.l[level].plane)) return rc;
  return down.receive(c);
}

}  // extern "C"
