// Host integration shim of the map point upkeep (include/defslam_hip.h: dsh_kfdb_*, dsh_mappoint_update):
//
//   KeyFrameStoreHIP<KeyFrameT> store(ctx)
//       the keyframe store in HBM: maps KeyFrame* to a slot and copies a keyframe up (descriptors, mvKeysUn octaves, camera centre,
//       pyramid) the first time a call sees it; Clear() for DefMap::clear on a reset.
//   ProcessNewKeyFrameHIP(ctx, store, pKF, recent)
//       drop-in for the map point loop of LocalMapping::ProcessNewKeyFrame (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:142-161, run by
//       DefLocalMapping::ProcessNewKeyFrame, Modules/Mapping/DefLocalMapping.cc:160-164): AddObservation for every good map point of the
//       keyframe that does not observe it yet, then UpdateNormalAndDepth and ComputeDistinctiveDescriptors of those points in one batch
//       (the points do not interact, so the batch is exact); the others go to `recent` (mlpRecentAddedMapPoints), as in the reference.
//   UpdateMapPointsHIP(ctx, store, points, what)
//       the two methods on a list of points: DefLocalMapping::CreateNewMapPoints (DefLocalMapping.cc:340-341) and
//       DefTracking::MonocularInitialization (DefTracking.cc:610-611) with DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH, DefMapPoint::Repose
//       (DefMapPoint.cc:122-126, from TriangularMesh.cc:192) with DSH_MP_NORMAL_DEPTH after RecalculatePosition.
// Both return the library's status (DSH_OK == 0; dsh_last_error(ctx) has the text); nothing is written to a map point then, though
// ProcessNewKeyFrameHIP has already added the observations, as the reference does before it updates.  Bad points are skipped.  A
// keyframe's bad flag is read again (isBad()) at every call that uses it.
//
// Like defslam_hip_shim.h the functions are templates over the reference's classes; the type-specific pieces are the accessors of
// `MapPointAccess<KeyFrameT, MapPointT>`: cv::Mat in DefSLAM (GetCameraCenter(), mDescriptors.ptr(j), GetWorldPos(), and writers of
// MapPoint's protected mDescriptor / mNormalVector / mfMaxDistance / mfMinDistance, which need a friend declaration there), plain
// arrays in the stand-ins of standin_mappoint_types.h.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../include/defslam_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
struct MapPointAccess {
  static void center(KeyFrameT* kf, float* Ow) { std::memcpy(Ow, kf->Ow, 3 * sizeof(float)); }
  static const uint8_t* descriptors(KeyFrameT* kf) { return kf->mDescriptors.data(); }   // N x 32, row j = mDescriptors.row(j)
  static void world_pos(MapPointT* p, float* x) { std::memcpy(x, p->pos, 3 * sizeof(float)); }
  static void descriptor(MapPointT* p, uint8_t* d) { std::memcpy(d, p->mDescriptor, 32); }
  static void set_descriptor(MapPointT* p, const uint8_t* d) { std::memcpy(p->mDescriptor, d, 32); }
  static void set_normal_and_depth(MapPointT* p, const float* n, float max_d, float min_d) {
    std::memcpy(p->mNormalVector, n, 3 * sizeof(float));
    p->mfMaxDistance = max_d;
    p->mfMinDistance = min_d;
  }
};

template <class KeyFrameT, class MapPointT>
class KeyFrameStoreHIP {
 public:
  explicit KeyFrameStoreHIP(dsh_ctx* ctx, int capacity = 64) { status_ = dsh_kfdb_create(ctx, capacity, &db_); }
  ~KeyFrameStoreHIP() {
    if (db_) dsh_kfdb_destroy(db_);
  }
  KeyFrameStoreHIP(const KeyFrameStoreHIP&) = delete;
  KeyFrameStoreHIP& operator=(const KeyFrameStoreHIP&) = delete;
  int status() const { return status_; }
  dsh_kfdb* db() { return db_; }
  int Clear() {
    slots_.clear();
    return dsh_kfdb_clear(db_);
  }
  // a keyframe the library put into the store itself (dsh_keyframe_create): its host object takes the slot
  void Adopt(KeyFrameT* kf, int32_t slot) { slots_[kf] = slot; }
  // the keyframe's slot, added on first sight; its bad flag refreshed.  -1 on failure (*rc has the status).
  int32_t Slot(KeyFrameT* kf, int* rc) {
    typename std::map<KeyFrameT*, int32_t>::iterator it = slots_.find(kf);
    int32_t s = -1;
    if (it != slots_.end()) {
      s = it->second;
    } else {
      typedef MapPointAccess<KeyFrameT, MapPointT> A;
      dsh_mp_keyframe k;
      std::memset(&k, 0, sizeof(k));
      A::center(kf, k.Ow);
      k.N = kf->N;
      std::vector<int32_t> oct(kf->N);
      for (int j = 0; j < kf->N; j++) oct[j] = kf->mvKeysUn[j].octave;
      k.desc = A::descriptors(kf);
      k.octave = oct.data();
      k.levels = kf->mnScaleLevels;
      k.scale_factors = kf->mvScaleFactors.data();
      k.bad = kf->isBad() ? 1 : 0;
      *rc = dsh_kfdb_add(db_, &k, &s);
      if (*rc != DSH_OK) return -1;
      slots_[kf] = s;
      return s;
    }
    *rc = dsh_kfdb_set_bad(db_, s, kf->isBad() ? 1 : 0);
    return *rc == DSH_OK ? s : -1;
  }

 private:
  dsh_kfdb* db_ = nullptr;
  int status_ = DSH_OK;
  std::map<KeyFrameT*, int32_t> slots_;
};

template <class KeyFrameT, class MapPointT>
int UpdateMapPointsHIP(dsh_ctx* ctx, KeyFrameStoreHIP<KeyFrameT, MapPointT>& store, const std::vector<MapPointT*>& points, int what) {
  typedef MapPointAccess<KeyFrameT, MapPointT> A;
  std::vector<MapPointT*> pts;
  for (size_t i = 0; i < points.size(); i++)
    if (points[i] && !points[i]->isBad()) pts.push_back(points[i]);   // both methods return at once on mbBad
  const int P = (int)pts.size();
  if (P == 0) return DSH_OK;
  std::vector<float> xyz(3 * (size_t)P), normal(3 * (size_t)P), maxd(P), mind(P);
  std::vector<int32_t> ptr(P + 1, 0), kf, idx, ref(P, 0), best(P), status(P);
  std::vector<uint8_t> desc(32 * (size_t)P);
  int rc = DSH_OK;
  for (int p = 0; p < P; p++) {
    MapPointT* mp = pts[p];
    A::world_pos(mp, &xyz[3 * (size_t)p]);
    A::descriptor(mp, &desc[32 * (size_t)p]);
    const std::map<KeyFrameT*, size_t> obs = mp->GetObservations();   // the reference's iteration order
    for (typename std::map<KeyFrameT*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) {
      const int32_t s = store.Slot(it->first, &rc);
      if (s < 0) return rc;
      kf.push_back(s);
      idx.push_back((int32_t)it->second);
    }
    ptr[p + 1] = (int32_t)kf.size();
    if ((what & DSH_MP_NORMAL_DEPTH) && !obs.empty()) {
      ref[p] = store.Slot(mp->GetReferenceKeyFrame(), &rc);
      if (ref[p] < 0) return rc;
    }
  }
  const bool d = (what & DSH_MP_DESCRIPTOR) != 0, g = (what & DSH_MP_NORMAL_DEPTH) != 0;
  rc = dsh_mappoint_update(ctx, store.db(), P, xyz.data(), ptr.data(), kf.data(), idx.data(), ref.data(), what, d ? desc.data() : nullptr,
                           d ? best.data() : nullptr, g ? normal.data() : nullptr, g ? maxd.data() : nullptr, g ? mind.data() : nullptr,
                           status.data());
  if (rc != DSH_OK) return rc;
  for (int p = 0; p < P; p++) {
    if (status[p] & DSH_MP_NO_OBS) continue;
    if (d && best[p] >= 0) A::set_descriptor(pts[p], &desc[32 * (size_t)p]);
    if (g) A::set_normal_and_depth(pts[p], &normal[3 * (size_t)p], maxd[p], mind[p]);
  }
  return DSH_OK;
}

template <class KeyFrameT, class MapPointT>
int ProcessNewKeyFrameHIP(dsh_ctx* ctx, KeyFrameStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* pKF, std::vector<MapPointT*>* recent = nullptr) {
  const std::vector<MapPointT*> vpMapPointMatches = pKF->GetMapPointMatches();
  std::vector<MapPointT*> update;
  for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
    MapPointT* pMP = vpMapPointMatches[i];
    if (!pMP || pMP->isBad()) continue;
    if (!pMP->IsInKeyFrame(pKF)) {
      pMP->AddObservation(pKF, i);
      update.push_back(pMP);
    } else if (recent) {
      recent->push_back(pMP);
    }
  }
  return UpdateMapPointsHIP(ctx, store, update, DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH);
}

}  // namespace defslam_hip
