// Stand-alone maps object (inspection / parity tests): the coordinate maps, kernel maps and neighbour tables of one
// sparse tensor as dgr_build_maps (kmap.hip) leaves them, in an arena of their own, and the entry points that read
// them back.
#include <string.h>

#include <algorithm>

#include "dgr_internal.h"

struct dgr_maps {
  dgr_ctx *ctx;
  DgrArena arena;  // private arena so the maps survive other calls on the ctx
  DgrMapSet ms;
  int32_t *coords_copy = nullptr;
  hipStream_t stream;
};

static int maps_create(dgr_ctx *ctx, const int32_t *coords, int64_t N, int D, int conv1_kernel_size, int flags,
                       dgr_maps **out, dgr_stream stream_) {
  DGR_REQUIRE(ctx && coords && out, "dgr_maps_create: NULL argument");
  DGR_REQUIRE((flags & ~(DGR_MAPS_LEAN | DGR_MAPS_NBR_LISTS)) == 0, "dgr_maps_create_ex: unknown flags 0x%x", flags);
  DGR_REQUIRE(!(flags & DGR_MAPS_NBR_LISTS) || ((flags & DGR_MAPS_LEAN) && D == 3),
              "dgr_maps_create_ex: DGR_MAPS_NBR_LISTS goes with DGR_MAPS_LEAN and D = 3");
  // lean: the arguments of dgr_resunet_forward_impl (net.hip) -- a 3-D net runs on neighbour tables with conv1 fused
  // with its search (no conv1 map), a 6-D net on lean rule-major maps
  const bool lean = (flags & DGR_MAPS_LEAN) != 0;
  hipStream_t stream = (hipStream_t)stream_;
  DGR_HIP_CHECK(hipSetDevice(ctx->device));
  dgr_maps *m = new dgr_maps();
  m->ctx = ctx;
  m->stream = stream;
  int rc = DGR_OK;
  do {
    m->coords_copy = m->arena.get<int32_t>((size_t)N * (D + 1));
    if (!m->coords_copy) { rc = DGR_ENOMEM; break; }
    if (hipMemcpyAsync(m->coords_copy, coords, (size_t)N * (D + 1) * sizeof(int32_t),
                       hipMemcpyDeviceToDevice, stream) != hipSuccess) { rc = DGR_EHIP; break; }
    rc = dgr_build_maps(m->arena, m->coords_copy, N, D, conv1_kernel_size, &m->ms, stream,
                        DgrMapsMode{lean, D == 3, (flags & DGR_MAPS_NBR_LISTS) != 0});
    if (rc != DGR_OK) break;
    int32_t flag = 0;
    if (hipMemcpyAsync(&flag, m->ms.overflow, sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) { rc = DGR_EHIP; dgr_set_error("maps sync failed"); break; }
    if (flag == 1) { dgr_set_error("duplicate coordinates in the sparse tensor input"); rc = DGR_EINVAL; break; }
    if (flag == 2) { dgr_set_error("kernel-map capacity exceeded"); rc = DGR_ENOMEM; break; }
  } while (0);
  if (rc != DGR_OK) {
    m->arena.release();
    delete m;
    return rc;
  }
  *out = m;
  return DGR_OK;
}

extern "C" int dgr_maps_create(dgr_ctx *ctx, const int32_t *coords, int64_t N, int D,
                               int conv1_kernel_size, dgr_maps **out, dgr_stream stream_) {
  return maps_create(ctx, coords, N, D, conv1_kernel_size, 0, out, stream_);
}

extern "C" int dgr_maps_create_ex(dgr_ctx *ctx, const int32_t *coords, int64_t N, int D, int conv1_kernel_size,
                                  int flags, dgr_maps **out, dgr_stream stream_) {
  return maps_create(ctx, coords, N, D, conv1_kernel_size, flags, out, stream_);
}

extern "C" void dgr_maps_destroy(dgr_maps *m) {
  if (!m) return;
  (void)hipDeviceSynchronize();
  m->arena.release();
  delete m;
}

static int level_of(int ts) { return ts == 1 ? 0 : ts == 2 ? 1 : ts == 4 ? 2 : ts == 8 ? 3 : -1; }

extern "C" int dgr_maps_get_coords(dgr_maps *m, int ts, int32_t *host_out, int64_t capacity,
                                   int64_t *n) {
  DGR_REQUIRE(m && n, "NULL argument");
  int l = level_of(ts);
  DGR_REQUIRE(l >= 0, "tensor stride %d not in {1,2,4,8}", ts);
  int32_t n32 = 0;
  DGR_HIP_CHECK(hipMemcpy(&n32, m->ms.cm[l].n_dev, sizeof(int32_t), hipMemcpyDeviceToHost));
  *n = n32;
  if (host_out) {
    DGR_REQUIRE(capacity >= (int64_t)n32 * m->ms.nc, "host buffer too small");
    const int nc = m->ms.nc;
    if (!m->ms.cm[l].canon) {
      DGR_HIP_CHECK(hipMemcpy(host_out, m->ms.cm[l].coords, (size_t)n32 * nc * sizeof(int32_t), hipMemcpyDeviceToHost));
    } else {   // rows back in first-occurrence order
      std::vector<int32_t> tmp((size_t)n32 * nc), canon(n32);
      DGR_HIP_CHECK(hipMemcpy(tmp.data(), m->ms.cm[l].coords, tmp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      DGR_HIP_CHECK(hipMemcpy(canon.data(), m->ms.cm[l].canon, canon.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int32_t p = 0; p < n32; ++p) memcpy(host_out + (size_t)canon[p] * nc, tmp.data() + (size_t)p * nc, nc * sizeof(int32_t));
    }
  }
  return DGR_OK;
}

extern "C" int dgr_maps_get_kernel_map(dgr_maps *m, int kind, int ts, int32_t *rule_ptr,
                                       int64_t rule_cap, int32_t *pair_in, int32_t *pair_out,
                                       int64_t pair_cap, int64_t *K, int64_t *P) {
  DGR_REQUIRE(m && K && P, "NULL argument");
  int l = level_of(ts);
  DGR_REQUIRE(l >= 0, "tensor stride %d not in {1,2,4,8}", ts);
  if (kind >= 3 && kind <= 5) {
    // D = 3 neighbour tables (kind 3: same stride, 4: ts -> 2 ts, 5: transposed 2 ts -> ts) as (k, in, out)
    // triplets sorted by (k, out) -- the layout the rule-major getter returns
    const DgrNbrTable *t = kind == 3 ? &m->ms.nsame[l] : (l < 3 ? (kind == 4 ? &m->ms.ndown[l] : &m->ms.nup[l]) : nullptr);
    DGR_REQUIRE(t && t->built, "no such neighbour table (kind %d, ts %d)", kind, ts);
    const DgrCoordMap &om = kind == 4 ? m->ms.cm[l + 1] : m->ms.cm[l];
    int32_t n_out = 0;
    DGR_HIP_CHECK(hipMemcpy(&n_out, om.n_dev, sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> tab((size_t)t->n_pad * 27);
    DGR_HIP_CHECK(hipMemcpy(tab.data(), t->nbr, tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    *K = 27;
    int64_t total = 0;
    for (int k = 0; k < 27; ++k) {
      if (rule_ptr && k < rule_cap) rule_ptr[k] = (int32_t)total;
      for (int o = 0; o < n_out; ++o) {
        const int32_t v = tab[(size_t)k * t->n_pad + o];
        if (v < 0) continue;
        if (pair_in && pair_out) {
          DGR_REQUIRE(total < pair_cap, "pair buffers too small");
          pair_in[total] = v;
          pair_out[total] = o;
        }
        ++total;
      }
    }
    if (rule_ptr) {
      DGR_REQUIRE(rule_cap >= 28, "rule_ptr buffer too small");
      rule_ptr[27] = (int32_t)total;
    }
    for (int64_t o = n_out; o < t->n_pad; ++o)
      for (int k = 0; k < 27; ++k) DGR_REQUIRE(tab[(size_t)k * t->n_pad + o] == -1, "neighbour table padding is not -1");
    *P = total;
    return DGR_OK;
  }
  const DgrKernelMap *km = nullptr;
  if (kind == 0) km = &m->ms.same[l];
  else if (kind == 1) km = &m->ms.conv1;
  else if (kind == 2 && l < 3) km = &m->ms.down[l];
  DGR_REQUIRE(km && km->built, "no such kernel map (kind %d, ts %d)", kind, ts);
  *K = km->K;
  int32_t total = 0;
  DGR_HIP_CHECK(hipMemcpy(&total, km->rule_ptr + km->K, sizeof(int32_t), hipMemcpyDeviceToHost));
  *P = total;
  if (rule_ptr) {
    DGR_REQUIRE(rule_cap >= km->K + 1, "rule_ptr buffer too small");
    DGR_HIP_CHECK(hipMemcpy(rule_ptr, km->rule_ptr, (size_t)(km->K + 1) * sizeof(int32_t),
                            hipMemcpyDeviceToHost));
  }
  if (pair_in && pair_out) {
    DGR_REQUIRE(pair_cap >= total, "pair buffers too small");
    DGR_REQUIRE(km->pair_out, "this build kept no pair_out for the map (kind %d, ts %d): read it raw", kind, ts);
    DGR_HIP_CHECK(hipMemcpy(pair_in, km->pair_in, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    DGR_HIP_CHECK(hipMemcpy(pair_out, km->pair_out, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost));
    // rows in first-occurrence numbering (coarse 6-D maps are numbered by bucket inside the library), pairs of a rule
    // sorted by output row in THAT numbering: the layout the getter documents
    const DgrCoordMap &cin = m->ms.cm[l], &cout = m->ms.cm[kind == 2 ? l + 1 : l];
    if (cin.canon || cout.canon) {
      auto fetch = [&](const DgrCoordMap &c, std::vector<int32_t> &v) -> int {
        if (!c.canon) return DGR_OK;
        int32_t n = 0;
        DGR_HIP_CHECK(hipMemcpy(&n, c.n_dev, sizeof(int32_t), hipMemcpyDeviceToHost));
        v.resize(n);
        DGR_HIP_CHECK(hipMemcpy(v.data(), c.canon, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return DGR_OK;
      };
      std::vector<int32_t> ci, co, rp(km->K + 1);
      DGR_CHECK(fetch(cin, ci));
      DGR_CHECK(fetch(cout, co));
      DGR_HIP_CHECK(hipMemcpy(rp.data(), km->rule_ptr, rp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      std::vector<std::pair<int32_t, int32_t>> tmp;
      for (int k = 0; k < km->K; ++k) {
        tmp.clear();
        for (int32_t q = rp[k]; q < rp[k + 1]; ++q)
          tmp.push_back({cout.canon ? co[pair_out[q]] : pair_out[q], cin.canon ? ci[pair_in[q]] : pair_in[q]});
        std::sort(tmp.begin(), tmp.end());
        for (size_t u = 0; u < tmp.size(); ++u) { pair_out[rp[k] + u] = tmp[u].first; pair_in[rp[k] + u] = tmp[u].second; }
      }
    }
  }
  return DGR_OK;
}

// ------------------------------------------------------------------------------------------
// raw read-back (test instrument): one array as it lies in memory, in the library's own numbering
// ------------------------------------------------------------------------------------------
extern "C" int dgr_maps_get_raw(dgr_maps *m, const char *kind, int ts, const char *field, void *host_out,
                                int64_t capacity_bytes, int64_t *count, int64_t *elem_bytes) {
  DGR_REQUIRE(m && kind && field && count && elem_bytes, "dgr_maps_get_raw: NULL argument");
  const int l = level_of(ts);
  DGR_REQUIRE(l >= 0, "tensor stride %d not in {1,2,4,8}", ts);
  DGR_HIP_CHECK(hipSetDevice(m->ctx->device));
  DGR_HIP_CHECK(hipStreamSynchronize(m->stream));
  const DgrMapSet &ms = m->ms;
  const auto is = [](const char *a, const char *b) { return strcmp(a, b) == 0; };
  const void *dev = nullptr;   // device array to copy ...
  int64_t n = 0, eb = 4;       // ... of n elements of eb bytes; or
  bool scalar = false;         // one host value
  int64_t value = 0;
  const auto rows_of = [](const DgrCoordMap &c, int64_t *rows) -> int {
    int32_t n32 = 0;
    DGR_HIP_CHECK(hipMemcpy(&n32, c.n_dev, sizeof(int32_t), hipMemcpyDeviceToHost));
    *rows = n32;
    return DGR_OK;
  };
  if (is(kind, "level")) {
    const DgrCoordMap &c = ms.cm[l];
    int64_t rows = 0;
    DGR_CHECK(rows_of(c, &rows));
    if (is(field, "coords")) { dev = c.coords; n = rows * ms.nc; }
    else if (is(field, "canon")) {
      DGR_REQUIRE(c.canon, "level ts %d is not renumbered: it has no canon", ts);
      dev = c.canon; n = rows;
    }
    else if (is(field, "table")) { dev = c.table; n = (int64_t)c.table_mask + 1; }
    else if (is(field, "n")) { scalar = true; value = rows; }
    else if (is(field, "mask")) { scalar = true; value = c.table_mask; }
    else DGR_REQUIRE(false, "no field '%s' in a level", field);
  } else if (is(kind, "same") || is(kind, "conv1") || is(kind, "down")) {
    const bool down = is(kind, "down");
    DGR_REQUIRE(!down || l < 3, "no strided map at ts %d", ts);
    DGR_REQUIRE(!is(kind, "conv1") || l == 0, "the conv1 map lives at ts 1");
    const DgrKernelMap *km = down ? &ms.down[l] : is(kind, "conv1") ? &ms.conv1 : &ms.same[l];
    DGR_REQUIRE(km->built, "this build made no '%s' map at ts %d", kind, ts);
    const DgrCoordMap &cin = ms.cm[l], &cout = ms.cm[down ? l + 1 : l];
    int32_t tot[2] = {0, 0};   // pairs, tiles
    DGR_HIP_CHECK(hipMemcpy(&tot[0], km->rule_ptr + km->K, sizeof(int32_t), hipMemcpyDeviceToHost));
    DGR_HIP_CHECK(hipMemcpy(&tot[1], km->tile_ptr + km->K, sizeof(int32_t), hipMemcpyDeviceToHost));
    const int64_t P = std::min<int64_t>(std::max<int64_t>(tot[0], 0), km->pair_cap);
    const int64_t T = std::min<int64_t>(std::max<int64_t>(tot[1], 0), km->tile_cap);
    if (is(field, "rule_ptr")) { dev = km->rule_ptr; n = km->K + 1; }
    else if (is(field, "tile_ptr")) { dev = km->tile_ptr; n = km->K + 1; }
    else if (is(field, "tile_desc")) { dev = km->tile_desc; n = 4 * T; }
    else if (is(field, "pair_in")) { dev = km->pair_in; n = P; }
    else if (is(field, "pair_out")) {
      DGR_REQUIRE(km->pair_out, "this build kept no pair_out for the '%s' map at ts %d", kind, ts);
      dev = km->pair_out; n = P;
    }
    else if (is(field, "pair_k")) {
      DGR_REQUIRE(km->pair_k, "this build kept no pair_k for the '%s' map at ts %d", kind, ts);
      dev = km->pair_k; n = P; eb = 2;
    }
    else if (is(field, "out_ptr")) { dev = km->out_ptr; n = cout.n_cap + 1; }
    else if (is(field, "out_pos")) { dev = km->out_pos; n = P; }
    else if (is(field, "in_ptr") || is(field, "in_pos")) {
      DGR_REQUIRE(km->in_ptr && km->in_pos, "the '%s' map at ts %d has no in-major CSR", kind, ts);
      if (is(field, "in_ptr")) { dev = km->in_ptr; n = cin.n_cap + 1; } else { dev = km->in_pos; n = P; }
    }
    else if (is(field, "pair_cap")) { scalar = true; value = km->pair_cap; }
    else if (is(field, "n_cap")) { scalar = true; value = cout.n_cap; }
    else if (is(field, "K")) { scalar = true; value = km->K; }
    else DGR_REQUIRE(false, "no field '%s' in a kernel map", field);
  } else if (is(kind, "nbr_same") || is(kind, "nbr_down") || is(kind, "nbr_up")) {
    DGR_REQUIRE(is(kind, "nbr_same") || l < 3, "no such neighbour table at ts %d", ts);
    const DgrNbrTable *t = is(kind, "nbr_same") ? &ms.nsame[l] : is(kind, "nbr_down") ? &ms.ndown[l] : &ms.nup[l];
    DGR_REQUIRE(t->built, "this build made no '%s' table at ts %d", kind, ts);
    if (is(field, "nbr")) { dev = t->nbr; n = t->n_pad * t->K; }
    else if (is(field, "n_pad")) { scalar = true; value = t->n_pad; }
    else if (is(field, "perm") || is(field, "cls_count") || is(field, "cls_cap")) {
      DGR_REQUIRE(t->perm && t->cls_count, "the '%s' table at ts %d has no parity classes", kind, ts);
      if (is(field, "perm")) { dev = t->perm; n = 8 * t->cls_cap; }
      else if (is(field, "cls_count")) { dev = t->cls_count; n = 8; }
      else { scalar = true; value = t->cls_cap; }
    }
    else DGR_REQUIRE(false, "no field '%s' in a neighbour table", field);
  } else {
    DGR_REQUIRE(false, "no kind '%s'", kind);
  }
  if (scalar) { n = 1; eb = 8; }
  *count = n;
  *elem_bytes = eb;
  if (!host_out) return DGR_OK;
  DGR_REQUIRE(capacity_bytes >= n * eb, "host buffer too small (%lld < %lld bytes)", (long long)capacity_bytes, (long long)(n * eb));
  if (scalar) {
    memcpy(host_out, &value, sizeof(int64_t));
  } else if (n > 0) {
    DGR_REQUIRE(dev, "field '%s' of '%s' at ts %d was not built", field, kind, ts);
    DGR_HIP_CHECK(hipMemcpy(host_out, dev, (size_t)(n * eb), hipMemcpyDeviceToHost));
  }
  return DGR_OK;
}
