// bge_spherecast.hpp — launch entry points of the sphere queries (bge_spherecast.hip; include/bge_world.h bge_world_sphere_cast*,
// bge_world_overlap_sphere).  They see the world the ray queries see and travel in the same RayParams (bge_raycast.hpp): `rays`
// holds the bge_sphere_cast or bge_sphere records, `n_rays` their number, `hits` the bge_ray_hit records of the closest cast.
#pragma once

#include "bge_raycast.hpp"

namespace bge {

// closest touch per cast: the body pass, then one thread per cast (ghosts, plane, the record)
hipError_t launch_sphere_cast_closest(hipStream_t stream, const RayParams& p);
// every touch: appends (cast, object code, fraction, normal) to p.all behind p.all_count (zeroed before the call by the caller)
hipError_t launch_sphere_cast_all(hipStream_t stream, const RayParams& p);
// overlap: appends (sphere, object code, distance) for every object within the sphere's radius of its centre; n is not written
hipError_t launch_sphere_overlap(hipStream_t stream, const RayParams& p);

} // namespace bge
