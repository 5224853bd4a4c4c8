// trange.h -- trajectory range query (PointPolygonTRangeQuery.java:53-177), see trange.hip.
#pragma once
#include "geohip_internal.h"

namespace geohip {
// the ctx's cached polygon plan of geohip_trange_classify and its device tables
void** ctx_tcache_slot(geohip_ctx* ctx);
// drop them (geohip_ctx_destroy, with the ctx's device selected)
void trange_cache_drop(geohip_ctx* ctx);
}  // namespace geohip
