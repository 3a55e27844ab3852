// host_check.cpp -- drives every member of the C++ mirror (vcp_host.hpp) and the vcp_dev_* path from a case file and
// writes back every field a caller can observe.  It holds no expectation of its own: tests/test_cpp_mirror_gpu.py writes
// the cases, computes what the references say and compares.
// Usage: host_check <case-file> <result-file>
// Container (tests/vcpbin.py reads and writes the same): "VCPBIN1\0", u32 record count, then per record
//   u16 name length, name, u8 dtype tag (0 u8, 1 i32, 2 i64, 3 f64), u64 element count, raw little-endian elements.
// A case is every record named "<case>/<field>"; "<case>/op" (u8 text) names the member to drive.  Results are
// "<case>/<field>" records as well.  Doubles travel as bits.
// Build: g++ -std=c++17 -Wall -Wextra -I include host_check.cpp -L vtkcloudpoint_amd -lvcp -Wl,-rpath,<dir>
#include <cstdio>
#include <cstring>
#include <memory>

#include "vcp_host.hpp"

using namespace vtkPointCloud;

namespace {

enum Tag : uint8_t { U8 = 0, I32 = 1, I64 = 2, F64 = 3 };
const size_t kSize[4] = {1, 4, 8, 8};

struct Rec {
  std::string name;
  uint8_t tag = U8;
  uint64_t count = 0;
  std::vector<uint8_t> bytes;
};

std::vector<Rec> g_in, g_out;

bool read_file(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  char magic[8];
  uint32_t nrec = 0;
  bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "VCPBIN1\0", 8) == 0 && std::fread(&nrec, 4, 1, f) == 1;
  for (uint32_t r = 0; ok && r < nrec; r++) {
    Rec rec;
    uint16_t nl = 0;
    ok = std::fread(&nl, 2, 1, f) == 1;
    if (!ok) break;
    rec.name.resize(nl);
    ok = (nl == 0 || std::fread(&rec.name[0], 1, nl, f) == nl) && std::fread(&rec.tag, 1, 1, f) == 1 && rec.tag <= F64 &&
         std::fread(&rec.count, 8, 1, f) == 1 && rec.count < (1ull << 32);
    if (!ok) break;
    rec.bytes.resize((size_t)rec.count * kSize[rec.tag]);
    ok = rec.bytes.empty() || std::fread(rec.bytes.data(), 1, rec.bytes.size(), f) == rec.bytes.size();
    g_in.push_back(std::move(rec));
  }
  std::fclose(f);
  return ok;
}

bool write_file(const char* path) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const uint32_t nrec = (uint32_t)g_out.size();
  bool ok = std::fwrite("VCPBIN1\0", 1, 8, f) == 8 && std::fwrite(&nrec, 4, 1, f) == 1;
  for (const Rec& rec : g_out) {
    const uint16_t nl = (uint16_t)rec.name.size();
    ok = ok && std::fwrite(&nl, 2, 1, f) == 1 && std::fwrite(rec.name.data(), 1, nl, f) == nl &&
         std::fwrite(&rec.tag, 1, 1, f) == 1 && std::fwrite(&rec.count, 8, 1, f) == 1 &&
         (rec.bytes.empty() || std::fwrite(rec.bytes.data(), 1, rec.bytes.size(), f) == rec.bytes.size());
  }
  return std::fclose(f) == 0 && ok;
}

template <class T> struct TagOf;
template <> struct TagOf<uint8_t> { static const Tag v = U8; };
template <> struct TagOf<int32_t> { static const Tag v = I32; };
template <> struct TagOf<int64_t> { static const Tag v = I64; };
template <> struct TagOf<double> { static const Tag v = F64; };

// one case's view of the input records and its result writer
struct Case {
  std::string name;
  const Rec* find(const std::string& field) const {
    const std::string full = name + "/" + field;
    for (const Rec& r : g_in)
      if (r.name == full) return &r;
    return nullptr;
  }
  bool has(const std::string& field) const { return find(field) != nullptr; }
  template <class T> std::vector<T> vec(const std::string& field) const {
    const Rec* r = find(field);
    if (!r) throw std::runtime_error("case " + name + " lacks " + field);
    if (r->tag != TagOf<T>::v) throw std::runtime_error("case " + name + ": dtype of " + field);
    std::vector<T> v((size_t)r->count);
    if (!v.empty()) std::memcpy(v.data(), r->bytes.data(), r->bytes.size());
    return v;
  }
  template <class T> T one(const std::string& field) const {
    std::vector<T> v = vec<T>(field);
    if (v.size() != 1) throw std::runtime_error("case " + name + ": " + field + " is not a scalar");
    return v[0];
  }
  template <class T> T one(const std::string& field, T dflt) const { return has(field) ? one<T>(field) : dflt; }
  std::string text(const std::string& field) const {
    std::vector<uint8_t> v = vec<uint8_t>(field);
    return std::string(v.begin(), v.end());
  }
  template <class T> void put(const std::string& field, const T* p, size_t n) const {
    Rec r;
    r.name = name + "/" + field;
    r.tag = TagOf<T>::v;
    r.count = n;
    r.bytes.resize(n * sizeof(T));
    if (n) std::memcpy(r.bytes.data(), p, n * sizeof(T));
    g_out.push_back(std::move(r));
  }
  template <class T> void put(const std::string& field, const std::vector<T>& v) const { put(field, v.data(), v.size()); }
  template <class T> void put1(const std::string& field, T v) const { put(field, &v, 1); }
  void put_text(const std::string& field, const std::string& s) const { put(field, (const uint8_t*)s.data(), s.size()); }
};

// a list of Point3D objects owned here, handed to the mirror as std::vector<Point3D*>
struct Points {
  std::vector<std::unique_ptr<Point3D>> own;
  std::vector<Point3D*> lst;
  int64_t index_of(const Point3D* p) const {
    for (size_t i = 0; i < own.size(); i++)
      if (own[i].get() == p) return (int64_t)i;
    return -1;
  }
};

// <prefix>.n points; every field that has a record <prefix>.<field> is set, the others keep Point3D's defaults
void set_fields(const Case& cs, const std::string& pre, size_t n, const std::vector<Point3D*>& p) {
  auto f64 = [&](const char* f, size_t w) {
    std::vector<double> v = cs.has(pre + "." + f) ? cs.vec<double>(pre + "." + f) : std::vector<double>();
    if (!v.empty() && v.size() != n * w) throw std::runtime_error("case " + cs.name + ": size of " + pre + "." + f);
    return v;
  };
  auto i32 = [&](const char* f) {
    std::vector<int32_t> v = cs.has(pre + "." + f) ? cs.vec<int32_t>(pre + "." + f) : std::vector<int32_t>();
    if (!v.empty() && v.size() != n) throw std::runtime_error("case " + cs.name + ": size of " + pre + "." + f);
    return v;
  };
  auto u8 = [&](const char* f) {
    std::vector<uint8_t> v = cs.has(pre + "." + f) ? cs.vec<uint8_t>(pre + "." + f) : std::vector<uint8_t>();
    if (!v.empty() && v.size() != n) throw std::runtime_error("case " + cs.name + ": size of " + pre + "." + f);
    return v;
  };
  const std::vector<double> motor = f64("motor", 2), xyz = f64("xyz", 3), dist = f64("Distance", 1), tmp = f64("tmp", 3),
                            matched = f64("matched", 3);
  const std::vector<int32_t> idb = i32("IDBeforeMerge"), cid = i32("clusterId"), pid = i32("pathId"), pc = i32("ptsCount"),
                             mn = i32("matchNum");
  const std::vector<uint8_t> shown = u8("ifShown"), cls = u8("isClassed"), key = u8("isKeyPoint"), im = u8("isMatched");
  for (size_t i = 0; i < n; i++) {
    Point3D& q = *p[i];
    if (!motor.empty()) { q.motor_x = motor[2 * i]; q.motor_y = motor[2 * i + 1]; }
    if (!xyz.empty()) { q.X = xyz[3 * i]; q.Y = xyz[3 * i + 1]; q.Z = xyz[3 * i + 2]; }
    if (!tmp.empty()) { q.tmp_X = tmp[3 * i]; q.tmp_Y = tmp[3 * i + 1]; q.tmp_Z = tmp[3 * i + 2]; }
    if (!matched.empty()) { q.matched_X = matched[3 * i]; q.matched_Y = matched[3 * i + 1]; q.matched_Z = matched[3 * i + 2]; }
    if (!dist.empty()) q.Distance = dist[i];
    if (!idb.empty()) q.IDBeforeMerge = idb[i];
    if (!cid.empty()) q.clusterId = cid[i];
    if (!pid.empty()) q.pathId = pid[i];
    if (!pc.empty()) q.ptsCount = pc[i];
    if (!mn.empty()) q.matchNum = mn[i];
    if (!shown.empty()) q.ifShown = shown[i] != 0;
    if (!cls.empty()) q.isClassed = cls[i] != 0;
    if (!key.empty()) q.isKeyPoint = key[i] != 0;
    if (!im.empty()) q.isMatched = im[i] != 0;
  }
}

Points load_points(const Case& cs, const std::string& pre) {
  Points P;
  const size_t n = (size_t)cs.one<int64_t>(pre + ".n");
  for (size_t i = 0; i < n; i++) {
    P.own.emplace_back(new Point3D());
    P.lst.push_back(P.own.back().get());
  }
  set_fields(cs, pre, n, P.lst);
  return P;
}

std::vector<Point3D> load_values(const Case& cs, const std::string& pre) {
  std::vector<Point3D> v((size_t)cs.one<int64_t>(pre + ".n"));
  std::vector<Point3D*> p;
  for (Point3D& q : v) p.push_back(&q);
  set_fields(cs, pre, v.size(), p);
  return v;
}

// every field of every point, as <prefix>.<field>
void dump_points(const Case& cs, const std::string& pre, const std::vector<const Point3D*>& p) {
  const size_t n = p.size();
  std::vector<double> motor(2 * n), xyz(3 * n), dist(n), tmp(3 * n), matched(3 * n);
  std::vector<int32_t> idb(n), cid(n), pid(n), pc(n), mn(n);
  std::vector<uint8_t> shown(n), cls(n), key(n), im(n);
  for (size_t i = 0; i < n; i++) {
    const Point3D& q = *p[i];
    motor[2 * i] = q.motor_x; motor[2 * i + 1] = q.motor_y;
    xyz[3 * i] = q.X; xyz[3 * i + 1] = q.Y; xyz[3 * i + 2] = q.Z;
    tmp[3 * i] = q.tmp_X; tmp[3 * i + 1] = q.tmp_Y; tmp[3 * i + 2] = q.tmp_Z;
    matched[3 * i] = q.matched_X; matched[3 * i + 1] = q.matched_Y; matched[3 * i + 2] = q.matched_Z;
    dist[i] = q.Distance;
    idb[i] = q.IDBeforeMerge; cid[i] = q.clusterId; pid[i] = q.pathId; pc[i] = q.ptsCount; mn[i] = q.matchNum;
    shown[i] = q.ifShown; cls[i] = q.isClassed; key[i] = q.isKeyPoint; im[i] = q.isMatched;
  }
  cs.put1<int64_t>(pre + ".n", (int64_t)n);
  cs.put(pre + ".motor", motor); cs.put(pre + ".xyz", xyz); cs.put(pre + ".Distance", dist);
  cs.put(pre + ".tmp", tmp); cs.put(pre + ".matched", matched);
  cs.put(pre + ".IDBeforeMerge", idb); cs.put(pre + ".clusterId", cid); cs.put(pre + ".pathId", pid);
  cs.put(pre + ".ptsCount", pc); cs.put(pre + ".matchNum", mn);
  cs.put(pre + ".ifShown", shown); cs.put(pre + ".isClassed", cls); cs.put(pre + ".isKeyPoint", key);
  cs.put(pre + ".isMatched", im);
}
void dump_points(const Case& cs, const std::string& pre, const std::vector<Point3D*>& p) {
  dump_points(cs, pre, std::vector<const Point3D*>(p.begin(), p.end()));
}
void dump_points(const Case& cs, const std::string& pre, const std::vector<Point3D>& v) {
  std::vector<const Point3D*> p;
  for (const Point3D& q : v) p.push_back(&q);
  dump_points(cs, pre, p);
}

void dump_db(const Case& cs, const std::string& pre, const DBImproved& db, long long it0) {
  cs.put1<int32_t>(pre + ".clusterAmount", db.clusterAmount);
  cs.put1<int32_t>(pre + ".pointsAmount", db.pointsAmount);
  cs.put1<int32_t>(pre + ".cf", db.cf);
  cs.put1<int64_t>(pre + ".iritatorNum", (int64_t)(DBImproved::iritatorNum - it0));
}

// -- one function per member ------------------------------------------------------------------------------------------

void op_dbscan(Context& ctx, const Case& cs, bool general) {
  Points P = load_points(cs, "pts");
  DBImproved db(ctx);
  db.cf = cs.one<int32_t>("cf", 0);
  const int calls = cs.one<int32_t>("calls", 1);
  for (int k = 0; k < calls; k++) {
    const long long it0 = DBImproved::iritatorNum;
    if (general)
      db.dbscanGeneral(P.lst, cs.one<double>("e"), cs.one<int64_t>("minWeight"), cs.one<double>("gate", -1.0),
                       cs.one<uint8_t>("usePtsCount", 0) != 0);
    else
      db.dbscan(P.lst, cs.one<double>("e"), cs.one<int32_t>("minPts"));
    const std::string pre = "call" + std::to_string(k);
    dump_points(cs, pre + ".pts", P.lst);
    dump_db(cs, pre, db, it0);
  }
}

void op_gdbscan(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  const vcp::GdbscanResult r = vcp::gdbscan(ctx, P.lst, cs.one<double>("e"), cs.one<int64_t>("minWeight"),
                                            cs.one<double>("gate", -1.0), cs.one<uint8_t>("usePtsCount", 0) != 0,
                                            cs.one<int32_t>("cfIn", 0));
  cs.put("labels", r.labels);
  cs.put("isCore", r.isCore);
  cs.put("hasNeighbourhood", r.hasNeighbourhood);
  cs.put1<int32_t>("cf", r.cf);
  dump_points(cs, "pts", P.lst);
}

void op_getDisP(const Case& cs) {
  Points P = load_points(cs, "pts");
  const long long it0 = DBImproved::iritatorNum;
  std::vector<double> d;
  for (size_t i = 0; i + 1 < P.lst.size(); i++) d.push_back(DBImproved::getDisP(*P.lst[i], *P.lst[i + 1]));
  cs.put("d", d);
  cs.put1<int64_t>("iritatorNum", (int64_t)(DBImproved::iritatorNum - it0));
}

void op_icp(Context& ctx, const Case& cs) {
  Points model = load_points(cs, "model"), data = load_points(cs, "data");
  Matrix R(cs.one<int32_t>("R.rows", 3), cs.one<int32_t>("R.cols", 3)), T(cs.one<int32_t>("T.rows", 3), cs.one<int32_t>("T.cols", 1));
  const std::vector<double> r0 = cs.vec<double>("R.mat"), t0 = cs.vec<double>("T.mat");
  if (r0.size() != R.mat.size() || t0.size() != T.mat.size()) throw std::runtime_error("case " + cs.name + ": R.mat / T.mat");
  R.mat = r0;
  T.mat = t0;
  ICP icp(ctx);
  icp.max_iter = cs.one<int32_t>("max_iter", icp.max_iter);
  try {
    icp.go_hell_ICP(model.lst, data.lst, R, T, cs.one<double>("e"));
    cs.put1<int32_t>("code", 0);
  } catch (const VcpException& e) {
    cs.put1<int32_t>("code", e.code);
  }
  cs.put("R.mat", R.mat);
  cs.put("T.mat", T.mat);
  cs.put1<double>("last_sse", icp.last_sse);
  cs.put1<int32_t>("last_iters", icp.last_iters);
}

void op_register(Context& ctx, const Case& cs, bool sim) {
  Points src = load_points(cs, "source"), tgt = load_points(cs, "target");
  const std::vector<int32_t> bases = cs.vec<int32_t>("bases");
  const bool outs = cs.one<uint8_t>("outputs", 1) != 0, mirror = cs.one<uint8_t>("mirror", 0) != 0;
  double M16[16];
  for (double& v : M16) v = -7.0;
  std::vector<int32_t> inliers(3, -5), score(3, -5);
  std::vector<double> scale(3, -5.0);
  ICP icp(ctx);
  int best;
  if (sim)
    best = icp.RegisterSimilarity(src.lst, tgt.lst, bases, cs.one<double>("scaleMin"), cs.one<double>("scaleMax"), mirror,
                                  cs.one<double>("inlierDist"), M16, outs ? &inliers : nullptr, outs ? &score : nullptr,
                                  outs ? &scale : nullptr);
  else
    best = icp.RegisterPairs(src.lst, tgt.lst, bases, cs.one<double>("lenTol"), mirror, cs.one<double>("inlierDist"), M16,
                             outs ? &inliers : nullptr, outs ? &score : nullptr);
  cs.put1<int32_t>("best", best);
  cs.put("M16", M16, 16);
  cs.put("inliers", inliers);
  cs.put("score", score);
  if (sim) cs.put("scale", scale);
}

// lists of point indices: <field>.start [K + 1] and <field>.idx
void dump_li(const Case& cs, const std::string& field, const std::vector<ClusObj>& cl, const Points& P) {
  std::vector<int64_t> start(1, 0), idx;
  std::vector<int32_t> ids;
  for (const ClusObj& c : cl) {
    for (const Point3D* p : c.li) idx.push_back(P.index_of(p));
    start.push_back((int64_t)idx.size());
    ids.push_back(c.clusId);
  }
  cs.put(field + ".start", start);
  cs.put(field + ".idx", idx);
  cs.put(field + ".clusId", ids);
}

void op_GetClusList(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  std::vector<ClusObj> cl((size_t)cs.one<int32_t>("K"));
  for (size_t k = 0; k < cl.size(); k++) cl[k].clusId = (int)k + 1;
  std::vector<Point3D> centers, centers2D;
  Tools::GetClusList(ctx, P.lst, centers, centers2D, cl);
  dump_points(cs, "centers", centers);
  dump_points(cs, "centers2D", centers2D);
  dump_li(cs, "li", cl, P);
  dump_points(cs, "pts", P.lst);
}

void op_Merge(Context& ctx, const Case& cs) {
  std::vector<Point3D> centers = load_values(cs, "centers");
  const std::map<int, int> d = Tools::MergeIDByDistance(ctx, centers, cs.one<double>("thre"));
  std::vector<int32_t> k, v;
  for (const auto& kv : d) { k.push_back(kv.first); v.push_back(kv.second); }
  cs.put("dict.keys", k);
  cs.put("dict.values", v);
  dump_points(cs, "centers", centers);
}

void op_getRectangles(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  const std::vector<int64_t> start = cs.vec<int64_t>("li.start"), idx = cs.vec<int64_t>("li.idx");
  std::vector<ClusObj> cl(start.empty() ? 0 : start.size() - 1);
  for (size_t k = 0; k < cl.size(); k++) {
    cl[k].clusId = (int)k + 1;
    for (int64_t t = start[k]; t < start[k + 1]; t++) cl[k].li.push_back(P.lst.at((size_t)idx.at((size_t)t)));
  }
  const std::vector<Tools::Rect2D> rects = Tools::getRectangles(ctx, cl, cs.one<uint8_t>("is3D") != 0);
  std::vector<int32_t> id;
  std::vector<double> len, cor;
  for (const Tools::Rect2D& r : rects) {
    id.push_back(r.clusID);
    len.push_back(r.len0);
    len.push_back(r.len1);
    cor.insert(cor.end(), r.corners, r.corners + 8);
  }
  cs.put("clusID", id);
  cs.put("len", len);
  cs.put("corners", cor);
}

void op_removeFilter(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  const std::vector<int32_t> f = cs.vec<int32_t>("filterID");
  std::vector<Point3D*> ds = P.lst;
  Tools::removeFilterPointFromClustering(ctx, ds, std::vector<int>(f.begin(), f.end()));
  std::vector<int64_t> kept;
  for (const Point3D* p : ds) kept.push_back(P.index_of(p));
  cs.put("kept", kept);
  dump_points(cs, "pts", P.lst);
}

void op_getClusterFromMotor(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  try {
    const BlockResult r = getClusterFromMotor(ctx, P.lst, cs.one<double>("tr"), cs.one<int32_t>("pts"), cs.one<int32_t>("ptsInCell"));
    cs.put1<int32_t>("code", 0);
    cs.put("clusForMerge", r.clusForMerge);
    const int32_t v[5] = {r.rows, r.cols, r.kept, r.delSum, r.clusterAmount};
    cs.put("rows_cols_kept_delSum_clusterAmount", v, 5);
    cs.put1<int64_t>("distEvals", (int64_t)r.distEvals);
  } catch (const VcpException& e) {
    cs.put1<int32_t>("code", e.code);
  }
  dump_points(cs, "pts", P.lst);
}

void op_match(Context& ctx, const Case& cs, bool unique) {
  std::vector<Point3D> centers = load_values(cs, "centers");
  const std::vector<double> truths = cs.vec<double>("truths"), M = cs.vec<double>("M");
  if (M.size() != 16) throw std::runtime_error("case " + cs.name + ": M");
  try {
    int cnt;
    if (unique) {
      const bool outs = cs.one<uint8_t>("outputs", 1) != 0;
      std::vector<int32_t> mid(2, -9), un(2, -9);
      cnt = MatchOneToOne(ctx, centers, truths, M.data(), cs.one<double>("matchDistance"), outs ? &mid : nullptr,
                          outs ? &un : nullptr);
      cs.put("matchedID", mid);
      cs.put("unmatchedTruths", un);
    } else {
      cnt = RecorrectMatchingPtsByDistance(ctx, centers, truths, M.data(), cs.one<double>("matchDistance"));
    }
    cs.put1<int32_t>("code", 0);
    cs.put1<int32_t>("count", cnt);
  } catch (const VcpException& e) {
    cs.put1<int32_t>("code", e.code);
  }
  dump_points(cs, "centers", centers);
}

void op_k_distance(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  const bool want = cs.one<uint8_t>("want_knn", 0) != 0;
  std::vector<int32_t> knn(5, -3);
  try {
    const std::vector<double> kd = k_distance(ctx, P.lst, cs.one<int32_t>("k"), cs.one<int32_t>("metric", VCP_L1_2D), want ? &knn : nullptr);
    cs.put1<int32_t>("code", 0);
    cs.put("kd", kd);
  } catch (const VcpException& e) {
    cs.put1<int32_t>("code", e.code);
  }
  cs.put("knn", knn);
}

void op_EpsTree(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  const bool given = cs.has("kdistGiven");
  const std::vector<double> kg = given ? cs.vec<double>("kdistGiven") : std::vector<double>();
  const EpsTreeResult r = EpsTree(ctx, P.lst, cs.one<int32_t>("k"), cs.one<double>("epsMax"), cs.one<int32_t>("metric", VCP_L1_2D),
                                  given ? &kg : nullptr);
  cs.put("kdist", r.kdist);
  cs.put("reach", r.reach);
  cs.put("mergeW", r.mergeW);
  cs.put("mergeA", r.mergeA);
  cs.put("mergeB", r.mergeB);
  cs.put1<double>("epsMax", r.epsMax);
  cs.put1<int32_t>("rounds", r.rounds);
  std::vector<int64_t> at;
  if (cs.has("eps_queries"))
    for (double e : cs.vec<double>("eps_queries")) at.push_back(r.clustersAt(e));
  cs.put("clustersAt", at);
}

// Context: release_workspace() between two calls, and the text an exception carries
void op_Context(Context& ctx, const Case& cs) {
  Points P = load_points(cs, "pts");
  DBImproved db(ctx);
  for (int k = 0; k < 2; k++) {
    for (Point3D* p : P.lst) { p->clusterId = 0; p->isClassed = false; p->isKeyPoint = false; }
    db.cf = 0;
    db.dbscan(P.lst, cs.one<double>("e"), cs.one<int32_t>("minPts"));
    dump_points(cs, "call" + std::to_string(k) + ".pts", P.lst);
    cs.put1<int32_t>("call" + std::to_string(k) + ".clusterAmount", db.clusterAmount);
    if (k == 0) ctx.release_workspace();
  }
  cs.put1<uint8_t>("get_nonnull", ctx.get() != nullptr);
  try {
    ctx.check(vcp_kdist(ctx.get(), nullptr, 1, 2, VCP_L1_2D, 0, nullptr, nullptr));  // NULL arrays and k = 0: an argument error
    cs.put1<int32_t>("code", 0);
  } catch (const VcpException& e) {
    cs.put1<int32_t>("code", e.code);
    cs.put_text("what", e.what());
    cs.put_text("last_error", vcp_last_error(ctx.get()));
  }
  ctx.check(VCP_OK);
}

// -- the device path of a host without a HIP binding: vcp_dev_alloc, vcp_h2d, the _dev call, vcp_d2h, vcp_dev_free --------

struct DevBuf {
  Context& c;
  void* p = nullptr;
  uint64_t bytes;
  DevBuf(Context& ctx, uint64_t b) : c(ctx), bytes(b) { c.check(vcp_dev_alloc(c.get(), b, &p)); }
  ~DevBuf() { if (p) vcp_dev_free(c.get(), p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void up(const void* src) { if (bytes) c.check(vcp_h2d(c.get(), p, src, bytes)); }
  void down(void* dst) { if (bytes) c.check(vcp_d2h(c.get(), dst, p, bytes)); }
};

void op_dev_dbscan(Context& ctx, const Case& cs) {
  const std::vector<double> coords = cs.vec<double>("coords");
  const int dim = cs.one<int32_t>("dim", 2);
  const int64_t n = (int64_t)coords.size() / dim;
  const bool classed = cs.has("in_classed");
  std::vector<uint8_t> cls = classed ? cs.vec<uint8_t>("in_classed") : std::vector<uint8_t>((size_t)n, 0);
  std::vector<int32_t> lab = classed ? cs.vec<int32_t>("labels") : std::vector<int32_t>((size_t)n, 0);
  std::vector<uint8_t> core((size_t)n, 0), out_cls((size_t)n, 0);
  if ((int64_t)cls.size() != n || (int64_t)lab.size() != n) throw std::runtime_error("case " + cs.name + ": sizes");
  DevBuf d_xy(ctx, 8ull * n * dim), d_cls(ctx, (uint64_t)n), d_lab(ctx, 4ull * n), d_core(ctx, (uint64_t)n), d_out(ctx, (uint64_t)n);
  d_xy.up(coords.data());
  d_cls.up(cls.data());
  d_lab.up(lab.data());
  d_core.up(core.data());
  d_out.up(out_cls.data());
  int32_t cf = 0;
  int64_t ev = 0;
  ctx.check(vcp_dbscan_dev(ctx.get(), (const double*)d_xy.p, n, dim, cs.one<int32_t>("metric", VCP_L1_2D), cs.one<double>("e"),
                           cs.one<int32_t>("minPts"), cs.one<int32_t>("cf", 0), classed ? (const uint8_t*)d_cls.p : nullptr,
                           (int32_t*)d_lab.p, (uint8_t*)d_core.p, (uint8_t*)d_out.p, &cf, &ev));
  d_lab.down(lab.data());
  d_core.down(core.data());
  d_out.down(out_cls.data());
  cs.put("labels", lab);
  cs.put("is_core", core);
  cs.put("is_classed", out_cls);
  cs.put1<int32_t>("cf", cf);
  cs.put1<int64_t>("evals", ev);
}

void op_dev_kdist(Context& ctx, const Case& cs) {
  const std::vector<double> coords = cs.vec<double>("coords");
  const int dim = cs.one<int32_t>("dim", 2), k = cs.one<int32_t>("k");
  const int64_t n = (int64_t)coords.size() / dim;
  if (k < 1) throw std::runtime_error("case " + cs.name + ": k");
  std::vector<double> kd((size_t)n, -1.0);
  std::vector<int32_t> knn((size_t)n * k, -1);
  DevBuf d_xy(ctx, 8ull * n * dim), d_kd(ctx, 8ull * n), d_knn(ctx, 4ull * n * k);
  d_xy.up(coords.data());
  d_kd.up(kd.data());
  d_knn.up(knn.data());
  ctx.check(vcp_kdist_dev(ctx.get(), (const double*)d_xy.p, n, dim, cs.one<int32_t>("metric", VCP_L1_2D), k, (double*)d_kd.p,
                          (int32_t*)d_knn.p));
  d_kd.down(kd.data());
  d_knn.down(knn.data());
  cs.put("kd", kd);
  cs.put("knn", knn);
}

void op_dev_centroids(Context& ctx, const Case& cs) {
  const std::vector<double> xyz = cs.vec<double>("xyz"), motor = cs.vec<double>("motor");
  const std::vector<int32_t> lab = cs.vec<int32_t>("labels");
  const int64_t n = (int64_t)lab.size();
  const int32_t K = cs.one<int32_t>("K");
  if ((int64_t)xyz.size() != 3 * n || (int64_t)motor.size() != 2 * n || K < 1) throw std::runtime_error("case " + cs.name + ": sizes");
  std::vector<double> c3(3 * (size_t)K, -1.0), c2(2 * (size_t)K, -1.0);
  std::vector<int64_t> cnt((size_t)K, -1);
  DevBuf d_xyz(ctx, 24ull * n), d_mot(ctx, 16ull * n), d_lab(ctx, 4ull * n), d_c3(ctx, 24ull * K), d_c2(ctx, 16ull * K), d_cnt(ctx, 8ull * K);
  d_xyz.up(xyz.data());
  d_mot.up(motor.data());
  d_lab.up(lab.data());
  d_c3.up(c3.data());
  d_c2.up(c2.data());
  d_cnt.up(cnt.data());
  ctx.check(vcp_centroids_dev(ctx.get(), (const double*)d_xyz.p, (const double*)d_mot.p, (const int32_t*)d_lab.p, n, K,
                              (double*)d_c3.p, (double*)d_c2.p, (int64_t*)d_cnt.p));
  d_c3.down(c3.data());
  d_c2.down(c2.data());
  d_cnt.down(cnt.data());
  cs.put("c3", c3);
  cs.put("c2", c2);
  cs.put("counts", cnt);
}

// argument rules of the four helpers; every device pointer passed on is one vcp_dev_alloc returned
void op_dev_args(Context& ctx, const Case& cs) {
  void* p0 = nullptr;
  cs.put1<int32_t>("alloc0", vcp_dev_alloc(ctx.get(), 0, &p0));
  cs.put1<uint8_t>("alloc0_nonnull", p0 != nullptr);
  cs.put1<int32_t>("free0", p0 ? vcp_dev_free(ctx.get(), p0) : VCP_ERR_ARG);
  void* p = nullptr;
  double host[4] = {1.5, -0.0, 3.25, 4.0}, back[4] = {0, 0, 0, 0};
  cs.put1<int32_t>("alloc_null_ctx", vcp_dev_alloc(nullptr, 32, &p));
  cs.put1<int32_t>("alloc_null_out", vcp_dev_alloc(ctx.get(), 32, nullptr));
  ctx.check(vcp_dev_alloc(ctx.get(), 32, &p));
  cs.put1<int32_t>("h2d_null_ctx", vcp_h2d(nullptr, p, host, 32));
  cs.put1<int32_t>("h2d_null_dst", vcp_h2d(ctx.get(), nullptr, host, 32));
  cs.put1<int32_t>("d2h_null_ctx", vcp_d2h(nullptr, back, p, 32));
  cs.put1<int32_t>("d2h_null_src", vcp_d2h(ctx.get(), back, nullptr, 32));
  cs.put1<int32_t>("free_null_ctx", vcp_dev_free(nullptr, p));
  cs.put1<int32_t>("free_null_ptr", vcp_dev_free(ctx.get(), nullptr));
  ctx.check(vcp_h2d(ctx.get(), p, host, 32));
  ctx.check(vcp_d2h(ctx.get(), back, p, 32));
  cs.put("roundtrip", back, 4);
  ctx.check(vcp_dev_free(ctx.get(), p));
}

void run_case(Context& ctx, const Case& cs) {
  const std::string op = cs.text("op");
  if (op == "DBImproved::dbscan") op_dbscan(ctx, cs, false);
  else if (op == "DBImproved::dbscanGeneral") op_dbscan(ctx, cs, true);
  else if (op == "DBImproved::getDisP") op_getDisP(cs);
  else if (op == "vcp::gdbscan") op_gdbscan(ctx, cs);
  else if (op == "ICP::go_hell_ICP") op_icp(ctx, cs);
  else if (op == "ICP::RegisterPairs") op_register(ctx, cs, false);
  else if (op == "ICP::RegisterSimilarity") op_register(ctx, cs, true);
  else if (op == "Tools::GetClusList") op_GetClusList(ctx, cs);
  else if (op == "Tools::MergeIDByDistance") op_Merge(ctx, cs);
  else if (op == "Tools::getRectangles") op_getRectangles(ctx, cs);
  else if (op == "Tools::removeFilterPointFromClustering") op_removeFilter(ctx, cs);
  else if (op == "getClusterFromMotor") op_getClusterFromMotor(ctx, cs);
  else if (op == "RecorrectMatchingPtsByDistance") op_match(ctx, cs, false);
  else if (op == "MatchOneToOne") op_match(ctx, cs, true);
  else if (op == "k_distance") op_k_distance(ctx, cs);
  else if (op == "EpsTree") op_EpsTree(ctx, cs);
  else if (op == "Context") op_Context(ctx, cs);
  else if (op == "dev:dbscan") op_dev_dbscan(ctx, cs);
  else if (op == "dev:kdist") op_dev_kdist(ctx, cs);
  else if (op == "dev:centroids") op_dev_centroids(ctx, cs);
  else if (op == "dev:args") op_dev_args(ctx, cs);
  else throw std::runtime_error("case " + cs.name + ": unknown op " + op);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: host_check <case-file> <result-file>\n");
    return 2;
  }
  if (!read_file(argv[1])) {
    std::fprintf(stderr, "host_check: cannot read %s\n", argv[1]);
    return 2;
  }
  int ncases = 0;
  try {
    Context ctx(0);
    for (const Rec& r : g_in) {
      if (r.name.size() < 4 || r.name.compare(r.name.size() - 3, 3, "/op") != 0) continue;
      Case cs;
      cs.name = r.name.substr(0, r.name.size() - 3);
      try {
        run_case(ctx, cs);
        cs.put1<int32_t>("threw", 0);
      } catch (const VcpException& e) {  // a member that threw where the case did not expect it: the test sees the code
        cs.put1<int32_t>("threw", e.code);
        cs.put_text("threw_what", e.what());
      }
      ncases++;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "host_check: %s\n", e.what());
    return 1;
  }
  if (!write_file(argv[2])) {
    std::fprintf(stderr, "host_check: cannot write %s\n", argv[2]);
    return 2;
  }
  std::printf("host_check: %d cases\n", ncases);
  return 0;
}
